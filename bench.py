"""bench.py -- the graded measurement of the hot path: forward 3D C2C FFT, 512^3 fp64, slab-decomposed over N GPUs.

  python bench.py --gpus 1 --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

One "step" = one forward transform (t0 YZ FFT -> t1 pack -> t2 RCCL all-to-all -> t3 X FFT) of the same device-resident
synthetic input (uniform [-1,1) re/im, seeded); the total problem is fixed at 512^3 (strong scaling: BASELINE.json quotes
512^3 at 1/2/4/8 GPUs).  Everything timed runs through the C-ABI of libdfft_mi355x (HIP kernels + RCCL).
Rank 0 prints ONE JSON line.

A plain run does what the headline figure needs: plan set-up (the placement tuning and, for N > 1, the choice between the
overlapped and the serial pipeline included), warm-up, the timed steps, --dump-outputs, the line.  --full then goes on to
measure and check the transform it timed: per-stage and per-kernel times, the round-trip and direct-DFT errors, the roofline
block (with this command's rocprofv3 counter passes unless --no-pmc), for N > 1 the serial pipeline's full exchange, and at
N = 1 the CPU baseline (unless --no-cpu-baseline: the reference's heFFTe stock backend, or the oracle where that is not built).
"""
from __future__ import annotations

import argparse
import json
import math
import os
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: 8.0 TB/s spec
# best 2 GiB -> 2 GiB copy measured on this GPU model by this repository (round 2: 5.95 TB/s over 280 copy configurations; round 5,
# tools/l2probe.hip: 5.73-5.82 TB/s for a plain persistent copy over 12 buffer pairs, 6.40 TB/s when both sides fit the Infinity
# Cache -- profiles/r05/README.md section 2) and the guide's own float4 copy figure (MI355X_MICROARCH.md: 6.29 TB/s); both are quoted
HBM_COPY_CEILING_GBS = 5950.0
HBM_GUIDE_COPY_GBS = 6290.0
DUMP_ELEMENTS = 1 << 21        # --dump-outputs: output elements kept over all ranks (fp64: 32 MiB of values + 16 MiB of indices)


def parse_size(s: str):
    p = [int(v) for v in s.lower().split("x")]
    if len(p) == 1:
        p = p * 3
    assert len(p) == 3
    return tuple(p)


def physical_cores() -> int:
    """Physical cores of this host (unique (socket, core) pairs in /proc/cpuinfo); hardware threads if that cannot be read."""
    try:
        pairs, phys, core = set(), None, None
        for line in Path("/proc/cpuinfo").read_text().splitlines():
            if line.startswith("physical id"):
                phys = line.split(":")[1].strip()
            elif line.startswith("core id"):
                core = line.split(":")[1].strip()
            elif not line.strip():
                if phys is not None and core is not None:
                    pairs.add((phys, core))
                phys = core = None
        if phys is not None and core is not None:
            pairs.add((phys, core))
        if pairs:
            return len(pairs)
    except Exception:
        pass
    return os.cpu_count() or 1


def _heffte_stock(sample_n: int, ranks: int, timeout: float):
    """One run of the reference's bundled heFFTe 2.1.0 stock-CPU benchmark (oracle/_ref/speed3d_c2c, built from the sources
    under /root/reference by oracle/Makefile): (GFlops/s, 'Time per run' line) or None."""
    exe = ROOT / "oracle" / "_ref" / "speed3d_c2c"
    mpirun = Path("/opt/conda/bin/mpirun")
    if not (exe.exists() and mpirun.exists()):
        return None
    try:
        env = dict(os.environ)
        env["LD_LIBRARY_PATH"] = str(exe.parent / "mpilib") + ":" + env.get("LD_LIBRARY_PATH", "")
        r = subprocess.run([str(mpirun), "--oversubscribe", "-np", str(ranks), str(exe), "stock", "double", str(sample_n), str(sample_n),
                            str(sample_n), "-slabs", "-p2p_pl"], capture_output=True, text=True, timeout=timeout, env=env,
                           cwd="/tmp")
        if r.returncode != 0:  # older launchers do not know --oversubscribe
            r = subprocess.run([str(mpirun), "-np", str(ranks), str(exe), "stock", "double", str(sample_n), str(sample_n),
                                str(sample_n), "-slabs", "-p2p_pl"], capture_output=True, text=True, timeout=timeout, env=env,
                               cwd="/tmp")
        perf = [l for l in r.stdout.splitlines() if l.strip().startswith("Performance:")]
        tim = [l for l in r.stdout.splitlines() if l.strip().startswith("Time per run:")]
        if r.returncode == 0 and perf:
            return float(perf[0].split()[1]), (tim[0].strip() if tim else "")
    except Exception:
        pass
    return None


def cpu_baseline():
    """CPU leg (rank 0, N=1 only): the reference's bundled heFFTe stock backend on the metric's own configuration
    (512^3 fp64 C2C), 256^3 as a second, smaller sample.  MPI ranks (= cores used, stated in the line): 16 -- on the GPU
    box's host (2 x EPYC 9575F, 128 cores) the stock backend gets SLOWER with more ranks at this size (512^3: 14.9 GFlop/s
    on 16 ranks, 10.5 on 32, 8.5 on 64, > 200 s on 128; profiles/r02/experiments/cpu_baseline_rank_sweep.log), so the
    fastest measured launch is the one reported, and it keeps the CPU work to ~15 s.  DFFT_CPU_BASELINE_RANKS overrides.
    Falls back to timing the C restatement of the pipeline (a port) when the reference build is absent."""
    threads = os.cpu_count() or 1
    cores = physical_cores()
    want = int(os.environ.get("DFFT_CPU_BASELINE_RANKS", "16"))
    ranks = 1
    while ranks * 2 <= min(cores, max(want, 1)):
        ranks *= 2
    t0 = time.perf_counter()
    main_run = _heffte_stock(512, ranks, 150.0)
    t_main = time.perf_counter() - t0
    if main_run is not None:
        out = {"value": main_run[0], "unit": "GFlops/s", "cores": ranks, "kind": "reference",
               "sample": f"heFFTe 2.1.0 stock backend (bundled with the reference), 512^3 fp64 C2C (the metric's configuration), "
                         f"mpirun -np {ranks} -slabs -p2p_pl, {main_run[1]}, whole benchmark {t_main:.1f} s "
                         f"(host: {cores} physical cores, {threads} hardware threads)"}
        small = _heffte_stock(256, ranks, 60.0)
        if small is not None:
            out["second_sample"] = {"value": small[0], "unit": "GFlops/s", "sample": f"256^3 fp64 C2C, same launch, {small[1]}"}
        return out
    small = _heffte_stock(256, ranks, 120.0)
    if small is not None:
        return {"value": small[0], "unit": "GFlops/s", "cores": ranks, "kind": "reference",
                "sample": f"heFFTe 2.1.0 stock backend (bundled with the reference), 256^3 fp64 C2C (512^3 did not finish in "
                          f"150 s), mpirun -np {ranks} -slabs -p2p_pl, {small[1]} (host: {cores} physical cores, {threads} "
                          f"hardware threads)"}
    from oracle import slab_oracle as so
    n = 128
    x = so.random_input((n, n, n), seed=3)
    t = time.perf_counter()
    so.c_slab_fft3d(x, (n, n, n), 1, +1)
    dt = time.perf_counter() - t
    return {"value": 5.0 * n ** 3 * math.log2(n ** 3) * 1e-9 / dt, "unit": "GFlops/s", "cores": 1, "kind": "port",
            "sample": f"oracle/slab_oracle.c (scalar C restatement), {n}^3 fp64 forward, 1 thread, {dt:.3f} s"}


def dump_outputs(dirname: str, out, count: int, rank: int, P: int) -> None:
    """--dump-outputs: this rank's forward output as the timed path left it, as (elements, 2) re / im pairs in the transform's own
    precision -- whole when it has at most DUMP_ELEMENTS / P elements, otherwise one seeded element from each of that many equal
    stretches of it, with the element indices (float64, exact) in a second file.  Names carry the rank when P > 1."""
    import numpy as np
    import torch
    d = Path(dirname)
    d.mkdir(parents=True, exist_ok=True)
    name = "forward_output" if P == 1 else f"forward_output_rank{rank}"
    vals = torch.view_as_real(out[:count])
    keep = max(1, DUMP_ELEMENTS // P)
    if count <= keep:
        np.save(d / f"{name}.npy", vals.cpu().numpy())
        return
    stride = count // keep
    idx = np.arange(keep, dtype=np.int64) * stride + np.random.default_rng(4242 + rank).integers(0, stride, size=keep)
    np.save(d / f"{name}_sample.npy", vals[torch.from_numpy(idx).to(vals.device)].cpu().numpy())
    np.save(d / f"{name}_sample_index.npy", idx.astype(np.float64))


def is_forward_zy_kernel(name: str) -> bool:
    """rocprofv3 kernel name of the FORWARD one-launch YZ stage, any variant: zy_chunk_kernel<PZ, PY, DIR = 1, PACK, LAZY[, SIGN = 1[, SIG]]>.
    (The inverse stage run rows first is <..., 1, false, true, -1>: same structure, other transform -- not t0 of a forward execute.  A
    template parameter added to the kernel once made this test miss every launch and the bench line's roofline.traffic came out null:
    tests/test_host_logic.py pins the names.)"""
    import re
    # (round 6 added SIG behind SIGN -- and the pattern missed every launch again until the names below were taken from a real trace)
    return "zy_chunk_kernel" in name and re.search(r">, 1(, (true|false))*(, 1(, (true|false))*)?>", name) is not None


def library_sha256() -> str | None:
    """sha256 of the native library this process loaded: ties profiles/hbm_traffic.json to the build it was measured on."""
    try:
        import hashlib
        from distributedfft_amd import _lib
        path = Path(os.environ.get("DFFT_LIB", str(_lib.LIB_PATH)))
        return hashlib.sha256(path.read_bytes()).hexdigest()
    except Exception:
        return None


def measured_traffic(key: str, kernel: str):
    """(bytes per launch, source) from profiles/hbm_traffic.json when it was measured on the library build that is loaded
    now, else (None, reason)."""
    tfile = ROOT / "profiles" / "hbm_traffic.json"
    if not tfile.exists():
        return None, "profiles/hbm_traffic.json not present"
    try:
        tr = json.loads(tfile.read_text())
        ent = tr.get(key, {})
        if kernel not in ent:
            return None, f"no PMC entry for {kernel} / {key}"
        want, have = ent.get("library_sha256"), library_sha256()
        if want is None or have is None or want != have:
            return None, (f"PMC summary {ent.get('source', 'profiles/')} was taken on another build of the library "
                          f"(sha256 {str(want)[:12]} vs loaded {str(have)[:12]}): re-run tools/profile_bench.sh")
        return ent[kernel]["hbm_bytes_per_launch"], ent.get("source", "profiles/")
    except Exception as e:
        return None, f"profiles/hbm_traffic.json unreadable: {e}"


# What the memory system of this chip delivers to plain streaming kernels (tools/l2probe.hip on MI355X: persistent kernel, one 512-thread
# workgroup per CU, 16 B per lane, non-temporal; profiles/r05/experiments/l2probe_time.log) -- 2 GiB buffers in HBM / 64 MiB cache-resident
STREAM_GBS = {"read_hbm": 7020.0, "read_cache_resident": 7520.0, "write_hbm": 5570.0, "write_cache_resident": 5820.0,
              "copy_hbm": 5780.0, "copy_cache_resident": 6400.0}


def fabric_block(t0_bytes, t0_s, x_bytes, x_s):
    """Counter bytes (FETCH_SIZE x 2 + WRITE_SIZE: what crosses the L2 <-> fabric boundary, Infinity-Cache hits included) over launch
    time, next to the stream rates the same fabric gives plain kernels: the SURVEY 8(d) fraction charges the t0 launch 2 S N/P bytes,
    but the launch moves twice that through the fabric (Z -> Y intermediate written to and read back from the Infinity Cache), so a
    'frac' of ~0.46 of 8 TB/s is ~7.4 TB/s of fabric traffic -- at the read-stream rate of the chip."""
    def one(b, t):
        if b is None or not t:
            return None
        r = b / t / 1e9
        return {"bytes": b, "GB/s": round(r, 1), "over_read_stream_hbm": round(r / STREAM_GBS["read_hbm"], 3),
                "over_read_stream_cache_resident": round(r / STREAM_GBS["read_cache_resident"], 3),
                "over_copy_hbm": round(r / STREAM_GBS["copy_hbm"], 3), "over_copy_cache_resident": round(r / STREAM_GBS["copy_cache_resident"], 3)}
    out = {"stream_rates_GB/s": STREAM_GBS, "stream_rates_source": "tools/l2probe.hip, profiles/r05/experiments/l2probe_time.log",
           "t0_launch": one(t0_bytes, t0_s), "x_pass": one(x_bytes, x_s)}
    if t0_bytes is not None and x_bytes is not None and t0_s and x_s:
        out["transform"] = one(t0_bytes + x_bytes, t0_s + x_s)
    return out


def live_traffic(args, nchunks: int):
    """roofline.traffic observed by THIS run: two short child runs of this command (2 steps) under `rocprofv3 --kernel-trace
    --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` (separate passes, as MI355X_MICROARCH.md prescribes; FETCH_SIZE doubled, KB -> bytes
    x1024), bytes per launch of the X-pass kernel and of the whole t0 stage.  Returns (dict, note); dict is None when rocprofv3
    is not there, a pass fails or takes too long -- the committed figure is the fall-back then."""
    import csv
    import glob
    import re
    import shutil
    import tempfile
    exe = shutil.which("rocprofv3")
    if exe is None:
        return None, "rocprofv3 not found"
    csv.field_size_limit(1 << 30)
    got = {}
    size = "x".join(str(v) for v in args.size)
    for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix="dfft_pmc_", dir="/tmp")
        try:
            cmd = [exe, "--kernel-trace", "--pmc", ctr, "--output-format", "csv", "-d", d, "--", sys.executable, str(Path(__file__).resolve()),
                   "--gpus", "1", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-pmc", "--size", size, "--precision", args.precision]
            env = dict(os.environ, TMPDIR="/tmp")
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=150, cwd="/tmp", env=env)
            files = glob.glob(d + "/**/*counter_collection.csv", recursive=True)
            if r.returncode != 0 or not files:
                return None, f"rocprofv3 --pmc {ctr} pass failed (rc {r.returncode})"
            x, zy, rows_, cols_ = [], [], [], []
            for row in csv.DictReader(open(max(files, key=lambda f: os.path.getsize(f)))):
                name, val = row["Kernel_Name"], float(row["Counter_Value"])
                if "dfft::" not in name:
                    continue
                if "TuneTransposedStore" in name and ", 1, false" in name:
                    x.append(val)                      # forward X pass (the tuning's probe launches move the same bytes)
                elif is_forward_zy_kernel(name):
                    zy.append(val)
                elif ", 1, false, dfft::TuneStreamIn>" in name:
                    rows_.append(val)                  # forward Z rows, one launch per cache chunk
                elif ", 1, false, dfft::TuneCols>" in name or ", 1, false, dfft::TuneColsStreamOut>" in name:
                    cols_.append(val)
            if not x:
                return None, f"no X-pass dispatch in the {ctr} pass"
            t0 = (sum(zy) / len(zy)) if zy else ((sum(rows_) / len(rows_) + sum(cols_) / len(cols_)) * nchunks if rows_ and cols_ else None)
            got[ctr] = (sum(x) / len(x), t0)
        except Exception as e:  # timeout, unreadable output ...
            return None, f"rocprofv3 --pmc {ctr} pass: {e}"
        finally:
            shutil.rmtree(d, ignore_errors=True)
    fx, ft = got["FETCH_SIZE"]
    wx, wt = got["WRITE_SIZE"]
    out = {"x_pass_bytes_per_launch": (2 * fx + wx) * 1024,
           "t0_stage_bytes_per_execute": None if ft is None or wt is None else (2 * ft + wt) * 1024,
           "source": "measured by this run: child runs of this command (2 steps) under rocprofv3 --kernel-trace --pmc FETCH_SIZE / "
                     "--pmc WRITE_SIZE (separate passes; FETCH_SIZE doubled per MI355X_MICROARCH.md, KB -> bytes x1024; fabric-side "
                     "counters, Infinity-Cache hits included)"}
    return out, "ok"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--size", type=parse_size, default=(512, 512, 512))
    ap.add_argument("--precision", choices=["fp64", "fp32"], default="fp64")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure and check what the headline figure does not need: stage and "
                         "kernel times, round-trip and direct-DFT errors, roofline, serial-pipeline diagnostic, CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave out the CPU baseline")
    ap.add_argument("--no-pmc", action="store_true",
                    help="with --full: do not measure roofline.traffic with a rocprofv3 counter pass of this very command (N = 1 "
                         "only); the committed profiles/hbm_traffic.json figure is used if it belongs to the loaded library")
    ap.add_argument("--dry-run", action="store_true",
                    help="control-plane check only (CPU tests): rendezvous, id broadcast, slab bookkeeping; no GPU work")
    ap.add_argument("--unfused", action="store_true", help="reference stage structure (separate pack / transpose)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (each rank's forward output, a fixed seeded "
                         "sample of it when large) as DIR/<name>.npy; the input is seeded, so runs can be compared output for output")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    # stdout carries exactly ONE line (the JSON): RCCL prints a version banner to stdout when a communicator is created,
    # so everything else this process (and the libraries it loads) writes to fd 1 is sent to stderr instead
    sys.stdout.flush()
    json_out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)

    import numpy as np
    import torch
    import torch.distributed as dist
    from distributedfft_amd import api

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("--gpus N > 1 must be launched with torch.distributed.run (one rank per GPU)")
        raise SystemExit(f"WORLD_SIZE={world} does not match --gpus {args.gpus}")
    # tests/test_multirank_cpu.py runs this file's multi-rank reporting code with the native plan objects replaced by
    # stubs (no FFT is computed there); that is the only situation in which tensors are not on a HIP device
    stub_mode = getattr(api, "_BENCH_STUB", False)
    if not args.dry_run and not stub_mode:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a HIP device: the product path has no CPU fallback")
        torch.cuda.set_device(local_rank % torch.cuda.device_count())
        dev = torch.device("cuda", torch.cuda.current_device())
    elif stub_mode:
        dev = torch.device("cpu")

    P = world
    comm = None
    exchange_backend = os.environ.get("DFFT_EXCHANGE", "rccl").lower()
    comm_fallback = None
    def note(msg):  # launch diagnostics, one line per rank, never on stdout
        print(f"[bench rank {rank}/{world}] {msg}", file=sys.stderr, flush=True)

    if P > 1:
        # control plane on gloo (barriers, max-reduce, id broadcast); the data plane (t2) is RCCL inside the library
        dist.init_process_group(backend="gloo", init_method="env://", rank=rank, world_size=world)
        if not args.dry_run and not stub_mode:
            # --gpus N means N distinct GPUs: ranks sharing a device would time something else under the same name.
            # (DFFT_BENCH_ALLOW_SHARED_GPU=1: the single-GPU functional tests of this flow, IPC back-ends only.)
            prop = torch.cuda.get_device_properties(dev)
            mine = f"{os.uname().nodename}/{api.device_pci_bus_id(torch.cuda.current_device())}"  # PCI address, not the ordinal
            idents = [None] * world
            dist.all_gather_object(idents, mine)
            note(f"device {torch.cuda.current_device()} of {torch.cuda.device_count()} visible: {prop.name} [{mine}]")
            if len(set(idents)) < world and os.environ.get("DFFT_BENCH_ALLOW_SHARED_GPU", "0") != "1":
                if rank == 0:
                    print(f"bench.py --gpus {world}: only {len(set(idents))} distinct device(s) behind {world} ranks: {idents}",
                          file=sys.stderr, flush=True)
                dist.barrier()
                dist.destroy_process_group()
                raise SystemExit(4)
        uid = torch.zeros(128, dtype=torch.uint8)
        if rank == 0:
            raw = bytes(range(128)) if args.dry_run else api.Comm.rccl_unique_id()
            uid = torch.frombuffer(bytearray(raw), dtype=torch.uint8).clone()
        dist.broadcast(uid, src=0)
        uid_bytes = bytes(uid.tolist())
        if not args.dry_run:
            # DFFT_EXCHANGE=ipc: hipIpc peer copies + rendezvous barriers instead of RCCL (also works with several ranks on
            # one GPU -- how this multi-rank path is exercised on a single-GPU box); default: RCCL over xGMI
            if exchange_backend in ("ipc", "ipc-async"):
                comm = api.Comm.ipc(P, rank, exchange_backend == "ipc-async")
            else:
                # ncclCommInitRank is a blocking collective: a rank that never arrives would hang the others forever, and
                # a hung rank can never reach the agreement below -- a watchdog turns that into a loud, non-zero exit
                import threading
                limit = float(os.environ.get("DFFT_RCCL_INIT_TIMEOUT_S", "180"))

                def _abort():
                    print(f"[bench rank {rank}/{world}] ncclCommInitRank did not return within {limit:.0f} s "
                          f"(DFFT_RCCL_INIT_TIMEOUT_S): aborting", file=sys.stderr, flush=True)
                    os._exit(5)
                dog = threading.Timer(limit, _abort)
                dog.daemon = True
                dog.start()
                try:
                    # ranks that share a device (only possible with DFFT_BENCH_ALLOW_SHARED_GPU=1, the single-GPU functional tests):
                    # RCCL refuses duplicate devices -- known from the PCI addresses gathered above, on every rank alike, so
                    # ncclCommInitRank is not called at all.  (Driving RCCL into that error on purpose worked 50 times out of 50 in
                    # round 5 but once in round 4 left a rank inside ncclCommInitRank until the watchdog fired, 190 s later.)
                    if not stub_mode and len(set(idents)) < world:
                        raise RuntimeError(f"RCCL needs one device per rank: {len(set(idents))} distinct device(s) behind {world} ranks")
                    comm = api.Comm.rccl(uid_bytes, P, rank)
                    info = comm.info()
                    note(f"ncclCommInitRank ok: RCCL reports {info['size']} ranks, this is rank {info['rank']} on device "
                         f"{info['device']}")
                    if info["size"] != P or info["rank"] != rank:
                        raise RuntimeError(f"RCCL communicator has {info['size']} ranks / rank {info['rank']}, expected {P} / {rank}")
                except Exception as e:  # RCCL unusable on this node: every rank falls back to the IPC communicator together
                    note(f"ncclCommInitRank FAILED: {e}")
                    if comm is not None:
                        comm.destroy()
                    comm, comm_fallback = None, f"RCCL communicator could not be created ({e})"
                finally:
                    dog.cancel()
                ok = torch.tensor([1.0 if comm is not None else 0.0], dtype=torch.float64)
                dist.all_reduce(ok, op=dist.ReduceOp.MIN)
                if ok.item() != 1.0:
                    if comm is not None:
                        comm.destroy()
                    comm_fallback = comm_fallback or "RCCL communicator could not be created on another rank"
                    exchange_backend = "ipc-async"
                    note("EXCHANGE FALLBACK: RCCL is not usable on every rank -- this run uses the stream-ordered hipIpc "
                         "communicator instead (config.exchange and exchange_fallback in the JSON line say so)")
                    comm = api.Comm.ipc(P, rank, True)
    if args.dry_run:
        tot, inr, counts = api.fft_mpi_init(args.size, 1, mpi_size=P, mpi_rank=rank)
        lay = api.exchange_layout(*args.size, P, rank, api.FORWARD)
        ok = tot == P and (P == 1 or uid_bytes == bytes(range(128)))
        t = torch.tensor([float(sum(lay.scount))], dtype=torch.float64)
        if P > 1:
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            dist.barrier()
            dist.destroy_process_group()
        if rank == 0:
            json_out.write(json.dumps({"dry_run": True, "ok": bool(ok), "n_gpus": P, "elements_exchanged": t.item(),
                                       "local_count": counts[0]}) + "\n")
            json_out.flush()
        return

    def barrier():
        if not stub_mode:
            torch.cuda.synchronize()
        if P > 1:
            dist.barrier()

    n0, n1, n2 = args.size
    N = n0 * n1 * n2
    cdt = torch.complex128 if args.precision == "fp64" else torch.complex64
    rdt = torch.float64 if args.precision == "fp64" else torch.float32
    S = 16 if args.precision == "fp64" else 8
    tot, inr, counts = api.fft_mpi_init(args.size, 1, mpi_size=P, mpi_rank=rank)
    if tot != P:
        raise SystemExit(f"{n0} planes cannot be split over {P} devices the way the reference does (got {tot})")
    count = counts[0]
    max_count = api.get_max_data_count(n0, n1, n2, P, rank == P - 1)

    # synthetic input of this rank's X-slab, resident in HBM before anything is timed
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234 + rank)
    a = torch.zeros(max_count, dtype=cdt, device=dev)
    re = torch.rand(count, generator=gen, device=dev, dtype=rdt) * 2 - 1
    im = torch.rand(count, generator=gen, device=dev, dtype=rdt) * 2 - 1
    a[:count] = torch.complex(re, im)
    del re, im
    b = torch.zeros(max_count, dtype=cdt, device=dev)
    flags = api.PLAN_INPUT_FROM_IN | (api.PLAN_UNFUSED if args.unfused else 0)
    overlap = P > 1 and not args.unfused and os.environ.get("DFFT_BENCH_OVERLAP", "1") != "0"
    if overlap:
        flags |= api.PLAN_OVERLAP  # exchange parts on a second stream behind the plane-chunked Z+Y passes
    plan = api.Plan(n0, n1, n2, a, b, comm, rank, P, api.FORWARD, flags)
    plan_setup = "dfft_plan_create"
    tune_report, plan_desc = None, ""
    if P == 1 and hasattr(plan, "tune"):
        # This process owns the GPU, so the placement walk may borrow what the library's shared-GPU defaults (a quarter of the free
        # memory, 32 candidates) do not: on some boxes 60+ GiB of consecutive allocations behave alike (profiles/r04/experiments/
        # tune_check_short_walk.log: 4 of 10 processes found no fast buffer within 32 candidates and ran at 1.94 instead of 1.87 ms).
        os.environ.setdefault("DFFT_TUNE_MEM_PCT", "70")
        os.environ.setdefault("DFFT_TUNE_TRIES", "128")
        plan.tune()  # plan-time measurement (FFTW_MEASURE-style, part of plan set-up, before any warm-up or timed step)
        plan_setup += (" + dfft_plan_tune (plan-time placement of the hand-over buffer: the X-pass kernel alone timed on "
                       "candidate allocations -- up to 128 / 70 % of the free memory, all returned -- before warm-up; results "
                       "bit-identical without it)")
        if hasattr(plan, "tune_report"):
            tune_report = plan.tune_report()
    if hasattr(plan, "describe"):
        plan_desc = plan.describe()

    # P > 1: the un-overlapped plan is both the diagnostic (full t2) and the referee -- the overlapped pipeline must
    # reproduce its result bit for bit on every rank, otherwise the timed loop falls back to it
    plan_s, b2, overlap_note, pipeline_probe_ms, referee_same = None, None, None, None, None
    referee_forms_note, referee_bits = None, None
    if overlap:
        try:
            b2 = torch.zeros(max_count, dtype=cdt, device=dev)
            plan_s = api.Plan(n0, n1, n2, a, b2, comm, rank, P, api.FORWARD, api.PLAN_INPUT_FROM_IN)
            barrier()
            plan.execute(api.EXEC_ASYNC)
            plan.sync()
            barrier()
            plan_s.execute(api.EXEC_ASYNC)
            plan_s.sync()
            barrier()
            same_bits = torch.equal(b2[:count], b[:count])
            # The two plans normally run the same kernels and must agree bit for bit.  Where they run different FORMS of the YZ stage
            # (dfft_plan_describe: the lazy one-launch stage agrees with two launches per chunk only to the last bit or two, by
            # construction) bit-equality cannot hold; a race in the overlapped pipeline corrupts whole blocks, so 1e-13 of max|X|
            # still catches what the referee is there for.
            forms_differ = (not stub_mode and hasattr(plan, "describe")
                            and plan.describe().split("yz_stage=")[1].split()[0] != plan_s.describe().split("yz_stage=")[1].split()[0])
            close = same_bits
            if not same_bits and not stub_mode:
                # (also where a pass of the overlapped plan runs another kernel of the same length -- e.g. a 1024-point fp32 Y axis whose
                # 64-row destination sub-blocks are below the DIF-split kernel's 128-row grain, tools/fuzz_parity.py: last bits differ)
                scale_r = b2[:count].abs().max().item()
                referee_rel = ((b2[:count] - b[:count]).abs().max().item() / scale_r) if scale_r > 0 else float("inf")
                referee_tol = 1e-13 if args.precision == "fp64" else 2e-6
                close = referee_rel <= referee_tol
                why = (f"run different forms of the YZ stage ({plan_s.describe().split('yz_stage=')[1].split()[0]} / "
                       f"{plan.describe().split('yz_stage=')[1].split()[0]}), which agree to the last bit or two by construction" if forms_differ
                       else "select different kernels for a pass (same transform, different last bits)")
                referee_forms_note = (f"the serial and the overlapped plan {why}: compared to {referee_tol:g} of max|X| instead of bit for bit "
                                      f"(max relative difference on this rank {referee_rel:.2e})")
            same_t = torch.tensor([1.0 if close else 0.0, 1.0 if same_bits else 0.0], dtype=torch.float64)
            dist.all_reduce(same_t, op=dist.ReduceOp.MIN)
            referee_same = same_t[0].item() == 1.0
            referee_bits = same_t[1].item() == 1.0
            if not referee_same:
                overlap_note = "overlapped result differed from the serial pipeline: timed the serial pipeline instead"
            elif not stub_mode:
                # both pipelines are valid: time a few steps of each and keep the faster one for the measured run (the
                # overlap wins when the exchange is asynchronous -- RCCL --, not when it is host-synchronising -- IPC)
                quick = []
                for pl in (plan, plan_s):
                    barrier()
                    tq = time.perf_counter()
                    for _ in range(5):
                        pl.execute(api.EXEC_NO_TIMING)
                    pl.sync()
                    barrier()
                    quick.append(time.perf_counter() - tq)
                tq = torch.tensor(quick, dtype=torch.float64)
                dist.all_reduce(tq, op=dist.ReduceOp.MAX)
                pipeline_probe_ms = {"overlapped": round(tq[0].item() / 5 * 1e3, 4), "serial": round(tq[1].item() / 5 * 1e3, 4)}
                if tq[1].item() < 0.97 * tq[0].item():
                    overlap_note = (f"serial pipeline was faster in a 5-step probe ({pipeline_probe_ms['serial']} vs "
                                    f"{pipeline_probe_ms['overlapped']} ms per step): timed the serial pipeline")
        except Exception as e:  # never lose the headline number to the overlap machinery
            overlap_note = f"overlap set-up failed ({e}): timed the serial pipeline instead"
        # every rank must take the same branch below (plan creation / destruction are collectives on the IPC communicators
        # and the two pipelines issue different message sequences): agree on the decision
        agree = torch.tensor([0.0 if overlap_note is None else 1.0], dtype=torch.float64)
        dist.all_reduce(agree, op=dist.ReduceOp.MAX)
        if agree.item() != 0.0 and overlap_note is None:
            overlap_note = "another rank left the overlapped pipeline: timed the serial pipeline instead"
        if overlap_note is not None:
            overlap = False
            if plan_s is None:
                b2 = torch.zeros(max_count, dtype=cdt, device=dev)
                plan_s = api.Plan(n0, n1, n2, a, b2, comm, rank, P, api.FORWARD, api.PLAN_INPUT_FROM_IN)
            plan.destroy()
            plan, b, plan_s, b2 = plan_s, b2, None, None

    # The timed steps run the production way: no stage-boundary events (each event record is a barrier packet that drains the
    # queue between two kernels, ~20 us per execute); the per-stage breakdown below comes from separate, untimed executes.
    for _ in range(args.warmup):
        plan.execute(api.EXEC_NO_TIMING)
    plan.sync()

    barrier()
    t_start = time.perf_counter()
    for _ in range(args.steps):
        plan.execute(api.EXEC_NO_TIMING)
    plan.sync()
    barrier()
    elapsed = time.perf_counter() - t_start
    if P > 1:
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    sec_per_step = elapsed / args.steps
    gflops = 5.0 * N * math.log2(N) * 1e-9 / sec_per_step
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, b, count, rank, P)  # before any untimed execute below touches b

    # A plain run ends here: its line carries the headline figure and what the set-up decided.  --full goes on to measure and
    # check the transform it timed.
    if args.full:
        # ---- per-stage / per-kernel breakdown from HIP events on the plan's stream (separate, untimed executes) ----
        stage, kern = [], []
        for _ in range(10):
            barrier()
            plan.execute(api.EXEC_ASYNC)
            stage.append(plan.stage_times())
            if not args.unfused:
                try:
                    kern.append(plan.kernel_times())
                except api.DfftError:
                    pass  # Z and Y launches interleaved per Infinity-Cache chunk: only t0 (Z+Y) and t3 (X) are separable
        stage = np.median(np.array(stage), axis=0)
        kern = np.median(np.array(kern), axis=0) if kern else None
        if P > 1:
            t = torch.tensor(np.concatenate([stage, kern if kern is not None else np.zeros(3)]), dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            stage = t[:4].numpy()
            kern = t[4:].numpy() if kern is not None else None

        # ---- P > 1: the same transform without overlap, to report the full (un-hidden) t2 and the per-link rate ----
        serial_stage = None
        same = None
        if overlap:
            try:
                ss = []
                for i in range(8):
                    barrier()
                    plan_s.execute(api.EXEC_ASYNC)
                    st = plan_s.stage_times()
                    if i >= 3:
                        ss.append(st)
                t = torch.tensor(np.median(np.array(ss), axis=0), dtype=torch.float64)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                serial_stage = t.numpy()
                same = bool(torch.equal(b2[:count], b[:count]))  # overlap must not change a single bit of the result
                plan_s.destroy()
                del b2
            except Exception as e:  # never lose the headline number to the diagnostic
                serial_stage, same = None, f"serial diagnostic failed: {e}"

        # ---- error: the driver's round-trip metric (fftSpeed3d_c2c.cpp:84-91) on the device, plus an oracle spot check ----
        fwd_out = b.clone()
        c = torch.zeros(max_count, dtype=cdt, device=dev)
        planb = api.Plan(n0, n1, n2, fwd_out, c, comm, rank, P, api.BACKWARD, api.PLAN_DEFAULT)
        barrier()
        planb.execute(api.EXEC_ASYNC)
        planb.sync()
        rt_err = float((a[:count] - c[:count] / N).abs().max().item())
        if P > 1:
            t = torch.tensor([rt_err], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            rt_err = float(t.item())
        planb.destroy()
        del c, fwd_out

        # ---- independent full-size check: X[k] = sum_n x[n] e^{-2 pi i k.n/N} evaluated directly (fp64, summed over the
        # ranks' slabs) for a few seeded k, against the element of the distributed result that should hold it ----
        ks = [(0, 0, 0), (1, 2, 3), (n0 // 2, n1 - 1, n2 // 3), (n0 - 1, n1 // 2 + 1, n2 - 1), (n0 // 3, n1 // 5, 1)]
        xl_blk, yl_blk = -(-n0 // P), -(-n1 // P)
        x_first, xl = rank * xl_blk, count // (n1 * n2)
        x3 = a[:count].reshape(xl, n1, n2)
        direct = torch.zeros(len(ks), 2, dtype=torch.float64)
        got = torch.zeros(len(ks), 2, dtype=torch.float64)
        two_pi = 2.0 * math.pi
        for i, (kx, ky, kz) in enumerate(ks):
            def phase(k, n, idx):
                ang = (-two_pi * ((k * idx) % n).to(torch.float64) / n)
                return torch.complex(torch.cos(ang), torch.sin(ang))
            ez = phase(kz, n2, torch.arange(n2, device=dev))
            ey = phase(ky, n1, torch.arange(n1, device=dev))
            ex = phase(kx, n0, torch.arange(x_first, x_first + xl, device=dev))
            v = ((x3.to(torch.complex128) @ ez) @ ey * ex).sum() if cdt == torch.complex128 else \
                (((x3 @ ez.to(cdt)).to(torch.complex128)) @ ey * ex).sum()
            direct[i, 0], direct[i, 1] = float(v.real), float(v.imag)
            d_owner = min(ky // yl_blk, P - 1)
            if rank == d_owner:
                e = b[((ky - d_owner * yl_blk) * n2 + kz) * n0 + kx]
                got[i, 0], got[i, 1] = float(e.real), float(e.imag)
        if P > 1:
            dist.all_reduce(direct, op=dist.ReduceOp.SUM)
            dist.all_reduce(got, op=dist.ReduceOp.SUM)
        spot_err = float(((direct - got).pow(2).sum(dim=1).sqrt().max() / direct.pow(2).sum(dim=1).sqrt().max().clamp_min(1e-300)).item())
        del x3

        # ---- context for the roofline fraction: what a plain device-to-device copy of one pass's bytes achieves right now ----
        copy_gbs = None
        if rank == 0 and not stub_mode:
            try:
                dst = torch.empty_like(a)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                for _ in range(2):
                    dst.copy_(a)
                e0.record()
                for _ in range(5):
                    dst.copy_(a)
                e1.record()
                torch.cuda.synchronize()
                copy_gbs = 2.0 * a.numel() * S / (e0.elapsed_time(e1) / 5 * 1e-3) / 1e9
                del dst
            except Exception:
                copy_gbs = None
    elif plan_s is not None:
        plan_s.destroy()  # kept through the timed steps for the serial diagnostic of --full

    result = None
    if args.full and rank == 0:
        local_bytes = 2.0 * S * (N / P)  # each compute stage reads + writes its N/P elements once
        names = ["fft_rows Z", "fft_cols Y(+pack)", "fft_cols X(+transpose)"]
        roof = None
        if kern is None and not args.unfused:
            # chunked Z+Y: the X-pass kernel is the single longest launch; its duration is stage t3 (HIP events) -- of the
            # serial pipeline when the overlapped one interleaves t3 with the tail of t2
            x_s = float(serial_stage[3]) if serial_stage is not None else float(stage[3])
            ach = local_bytes / x_s / 1e9
            zy = 2 * local_bytes / float(stage[0]) / 1e9
            roof = {"bound": "hbm", "kernel": names[2], "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": round(ach / HBM_PEAK_GBS, 4), "frac_of_copy_ceiling": round(ach / HBM_COPY_CEILING_GBS, 4),
                    "frac_of_guide_copy_figure": round(ach / HBM_GUIDE_COPY_GBS, 4),
                    "traffic": None, "algorithmic_bytes_per_launch": local_bytes,
                    "device_copy_of_same_bytes_GB/s": None if copy_gbs is None else round(copy_gbs, 1),
                    "avg_launch_ms": round(x_s * 1e3, 4),
                    "zy_stage": {"note": "Z-row and Y-column kernels interleaved per 256 MiB Infinity-Cache chunk",
                                 "ms": round(float(stage[0]) * 1e3, 4), "algorithmic_GB/s": round(zy, 1),
                                 "frac_of_peak": round(zy / HBM_PEAK_GBS, 4),
                                 "as_one_stage_GB/s": round(zy / 2, 1),  # t0 read once + written once
                                 "as_one_stage_frac_of_peak": round(zy / 2 / HBM_PEAK_GBS, 4)},
                    "local_pipeline": {"bytes": 2 * local_bytes, "GB/s": round(2 * local_bytes / float(stage[0] + stage[1] + stage[3]) / 1e9, 1)}}
            key = f"{n0}x{n1}x{n2}_{args.precision}_P{P}"
            roof["traffic"], roof["traffic_source"] = measured_traffic(key, names[2])
            zt, zsrc = measured_traffic(key, "t0 chunk kernels (Z rows + Y columns)")
            committed = {"x_pass": roof["traffic"], "t0_stage": zt, "source": roof["traffic_source"]}
            if P == 1 and not args.no_pmc and not stub_mode:
                # the counters of THIS run (a child run of this command under rocprofv3); the committed summary stays in the line
                import re
                m = re.search(r"chunks=(\d+)x", plan_desc)
                live, note = live_traffic(args, int(m.group(1)) if m else 1)
                if live is not None:
                    roof["traffic"], roof["traffic_source"] = live["x_pass_bytes_per_launch"], live["source"]
                    if live["t0_stage_bytes_per_execute"] is not None:
                        zt, zsrc = live["t0_stage_bytes_per_execute"], live["source"]
                    roof["traffic_committed_profile"] = committed
                else:
                    roof["traffic_live_note"] = note
            roof["zy_stage"]["traffic"] = zt  # fabric bytes of the whole t0 stage (all chunk launches of one execute)
            if zt is None:
                roof["zy_stage"]["traffic_note"] = zsrc
            if "yz_stage=one-launch" in plan_desc and float(stage[0]) > x_s:
                # t0 is ONE launch now (dfft_zy.hip) and the longest one of the transform: it is the dominant kernel.  SURVEY 8(d)
                # charges the t0 stage 2 S N/P algorithmic bytes (read once, written once); inside, the launch makes two passes
                # over the data (Z rows, Y columns), which is why its fabric traffic is twice that.
                t0_s = float(stage[0])
                xroof = roof
                xroof.pop("zy_stage", None)
                roof = {"bound": "hbm", "kernel": "zy_chunk_kernel (t0: Z rows + Y columns of every Infinity-Cache chunk in one persistent launch)",
                        "achieved": round(local_bytes / t0_s / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": round(local_bytes / t0_s / 1e9 / HBM_PEAK_GBS, 4), "traffic": zt,
                        "traffic_source": xroof.get("traffic_source") if zt is not None else zsrc,
                        "algorithmic_bytes_per_launch": local_bytes, "avg_launch_ms": round(t0_s * 1e3, 4),
                        "passes_inside_the_launch": 2, "rate_of_its_two_passes_GB/s": round(2 * local_bytes / t0_s / 1e9, 1),
                        "frac_of_its_two_passes": round(2 * local_bytes / t0_s / 1e9 / HBM_PEAK_GBS, 4),
                        "device_copy_of_same_bytes_GB/s": None if copy_gbs is None else round(copy_gbs, 1),
                        "x_pass": xroof,
                        "local_pipeline": xroof.get("local_pipeline")}
                roof["fabric"] = fabric_block(zt, t0_s, xroof.get("traffic"), x_s)
        if kern is not None:
            k = int(np.argmax(kern))
            ach = local_bytes / kern[k] / 1e9
            roof = {"bound": "hbm", "kernel": names[k], "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": round(ach / HBM_PEAK_GBS, 4), "frac_of_copy_ceiling": round(ach / HBM_COPY_CEILING_GBS, 4),
                    "frac_of_guide_copy_figure": round(ach / HBM_GUIDE_COPY_GBS, 4),
                    "traffic": None, "algorithmic_bytes_per_launch": local_bytes,
                    "device_copy_of_same_bytes_GB/s": None if copy_gbs is None else round(copy_gbs, 1),
                    "avg_launch_ms": round(float(kern[k]) * 1e3, 4),
                    "all_kernels": {n: {"ms": round(float(t_) * 1e3, 4), "GB/s": round(local_bytes / t_ / 1e9, 1)}
                                    for n, t_ in zip(names, kern)},
                    "local_pipeline": {"bytes": 2 * local_bytes, "GB/s": round(2 * local_bytes / float(stage[0] + stage[1] + stage[3]) / 1e9, 1)}}
            roof["traffic"], roof["traffic_source"] = measured_traffic(f"{n0}x{n1}x{n2}_{args.precision}_P{P}", names[k])
        total_stage = float(sum(stage))
    if rank == 0:
        result = {
            "metric": "GFlops/s forward 3D C2C (5 N log2 N), 512^3 fp64" if args.size == (512, 512, 512) and args.precision == "fp64"
                      else f"GFlops/s forward 3D C2C (5 N log2 N), {n0}x{n1}x{n2} {args.precision}",
            "value": round(gflops, 2), "unit": "GFlops/s", "n_gpus": P, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(sec_per_step * 1e3, 4), "higher_is_better": True, "scaling": "strong",
            "vs_baseline": None, "dtype": "f64" if args.precision == "fp64" else "f32", "data": "synthetic",
            "config": {"workload": f"{n0}x{n1}x{n2} C2C {args.precision} forward, slab decomposition over {P} GPU(s), "
                                   f"{'fused' if not args.unfused else 'unfused'} pipeline, input resident in HBM",
                       "parallelism": f"slab{P}", "plan_setup": plan_setup, "plan": plan_desc,
                       "exchange": "none (P=1)" if P == 1 else
                                   ("hipIpc peer copies + rendezvous barriers (DFFT_EXCHANGE=ipc)" if exchange_backend == "ipc"
                                    else "hipIpc peer copies + stream-ordered flag words (DFFT_EXCHANGE=ipc-async)"
                                    if exchange_backend == "ipc-async" else "RCCL grouped send/recv over xGMI") +
                                   (", X-plane parts overlapped with t0 on a second stream (stages_ms.t2 = exposed part)" if overlap else "")},
        }
        if args.full:
            result.update({
                "max_error": rt_err / 1e7, "roundtrip_abs_error": rt_err,
                "direct_dft_spot_check_rel_error": spot_err,  # 5 output elements against the defining sum over all ranks' input
                "stages_ms": {"t0": round(float(stage[0]) * 1e3, 4), "t1": round(float(stage[1]) * 1e3, 4),
                              "t2": round(float(stage[2]) * 1e3, 4), "t3": round(float(stage[3]) * 1e3, 4)},
                "t2_fraction": round(float(stage[2]) / total_stage, 4) if total_stage > 0 else None,
                "roofline": roof,
            })
        result["reference_published"] = {"value": 644.112, "unit": "GFlops/s", "config": "512^3 fp64, 4 ranks, unnamed AMD GPUs "
                                         "(README.md:54 of the reference); comparable only at n_gpus=4"}
        if tune_report is not None:
            result["plan_tune"] = tune_report  # X-pass kernel time per candidate hand-over buffer, the one kept, and its re-timing
        if P == 4 and args.size == (512, 512, 512) and args.precision == "fp64":
            result["vs_baseline"] = round(gflops / 644.112, 3)
        if P > 1:
            if args.full:
                pair = S * N / (P * P)
                t2_full = float(serial_stage[2]) if serial_stage is not None else float(stage[2])
                result["xgmi"] = {"pair_chunk_bytes": pair, "t2_full_ms": round(t2_full * 1e3, 4),
                                  "achieved_GB/s_per_link": round(pair / t2_full / 1e9, 1) if t2_full > 0 else None,
                                  "peak_GB/s_per_link": 153.0}
                if overlap:
                    result["stages_ms_without_overlap"] = None if serial_stage is None else {
                        "t0": round(float(serial_stage[0]) * 1e3, 4), "t1": round(float(serial_stage[1]) * 1e3, 4),
                        "t2": round(float(serial_stage[2]) * 1e3, 4), "t3": round(float(serial_stage[3]) * 1e3, 4)}
                    result["overlap_result_bit_identical"] = same
                    if referee_forms_note is not None:
                        result["overlap_result_within_referee_tolerance"] = referee_same
                elif referee_same is not None:
                    result["overlap_result_bit_identical"] = referee_bits  # the referee's findings before the fallback
                    if referee_forms_note is not None:
                        result["overlap_result_within_referee_tolerance"] = referee_same
            result["pipeline"] = "overlapped" if overlap else "serial"
            if comm_fallback is not None:
                result["exchange_fallback"] = comm_fallback
            if overlap_note is not None:
                result["overlap_fallback"] = overlap_note
            if referee_forms_note is not None:
                result["overlap_referee"] = referee_forms_note
            if pipeline_probe_ms is not None:
                result["pipeline_probe_ms_per_step"] = pipeline_probe_ms
        if args.full and P == 1 and not args.no_cpu_baseline:
            result["cpu_baseline"] = cpu_baseline()
    plan.destroy()
    if comm is not None:
        comm.destroy()
    if P > 1:
        dist.barrier()
        dist.destroy_process_group()
    if result is not None:
        json_out.write(json.dumps(result) + "\n")
        json_out.flush()


if __name__ == "__main__":
    main()
