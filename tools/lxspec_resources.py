"""Register / scratch / LDS / occupancy of the long 1-D real cross-spectrum (csrc/dfft_lxspec.hip): the kernels of every instantiation
group -- pass A (factor length N x fp64 / fp32 x two-real / per-real accesses) and the accumulating Mid kernel (N > 64 x fp64 / fp32) -- and
the reduction, pad and multiply-accumulate kernels of the dispatcher unit, from the compiler's -Rpass-analysis=kernel-resource-usage
remarks (no GPU needed).  The first line carries the sha256 of dfft_lxspec.hip and dfft_lxspec.h, so tests/test_rxspec1d_long_host.py
can tell whether the inventory belongs to the sources in the tree.

  python tools/lxspec_resources.py [out.txt]        one line per kernel, sorted by length
  python tools/lxspec_resources.py --all [out.txt]  ... with lxspec_fused_ok overridden to build every Mid kernel (to find the spilling ones)"""
import hashlib
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from distributedfft_amd.build import NUM_INST_GROUPS as GROUPS  # noqa: E402

CSRC = ROOT / "distributedfft_amd" / "csrc"
SOURCES = ("dfft_lxspec.hip", "dfft_lxspec.h")


def sources_sha256():
    h = hashlib.sha256()
    for name in SOURCES:
        h.update((CSRC / name).read_bytes())
    return h.hexdigest()


def factor_lengths():
    return sorted({b << a for b in (1, 3, 5) for a in range(12) if 64 <= b << a <= 2048} | {81, 125})


def group_rows(g, everything=False):
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{ROOT / 'include'}", f"-I{CSRC}",
           f"-DDFFT_INST_GROUP={g}", "-Rpass-analysis=kernel-resource-usage", "-c", str(CSRC / "dfft_lxspec.hip"), "-o", "/dev/null"]
    if everything:  # lxspec_fused_ok lets every length through
        cmd.insert(1, "-DDFFT_LXSPEC_BUILD_ALL")
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-3000:])
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (.*?) \[-Rpass", line)
        if not m:
            continue
        text = m.group(1).strip()
        f = re.match(r"Function Name: _ZN4dfft\d+lxspec_a_kernelI15HIP_vector_typeI(d|f)Lj2EENS_4PlanILi(\d+)ELi(\d+)E.*?EELb([01])EEEv", text)
        if f:
            cur = {"kind": "lxspec_a", "type": "f64" if f.group(1) == "d" else "f32", "N": int(f.group(2)), "E": int(f.group(3)),
                   "variant": "vec" if f.group(4) == "1" else "real"}
            rows.append(cur)
            continue
        f = re.match(r"Function Name: _ZN4dfft\d+lxspec_mid_kernelI15HIP_vector_typeI(d|f)Lj2EENS_4PlanILi(\d+)ELi(\d+)E", text)
        if f:
            cur = {"kind": "lxspec_mid", "type": "f64" if f.group(1) == "d" else "f32", "N": int(f.group(2)), "E": int(f.group(3)), "variant": "any"}
            rows.append(cur)
            continue
        f = re.match(r"Function Name: _ZN4dfft\d+(lxspec_reduce|lxspec_pad|lxspec_mac)_kernelI(.*)EEv", text)
        if f:
            a = f.group(2)
            cur = {"kind": f.group(1), "type": "f64" if (a.startswith("d") or "HIP_vector_typeIdLj2E" in a) else "f32", "N": 0, "E": 0, "variant": "any"}
            rows.append(cur)
            continue
        if text.startswith("Function Name:"):
            cur = None
            continue
        if cur is None:
            continue
        for key, pat in (("vgpr", r"^VGPRs: (\d+)"), ("agpr", r"^AGPRs: (\d+)"), ("scratch", r"^ScratchSize \[bytes/lane\]: (\d+)"),
                         ("lds", r"^LDS Size \[bytes/block\]: (\d+)"), ("occ", r"^Occupancy \[waves/SIMD\]: (\d+)")):
            mm = re.match(pat, text)
            if mm:
                cur[key] = int(mm.group(1))
    return rows


def main():
    args = [a for a in sys.argv[1:] if a != "--all"]
    everything = "--all" in sys.argv[1:]
    with ThreadPoolExecutor(max_workers=min(GROUPS + 1, os.cpu_count() or 4, 16)) as ex:
        rows = [r for rs in ex.map(lambda g: group_rows(g, everything), range(GROUPS + 1)) for r in rs]
    rows.sort(key=lambda r: (r["N"], r["kind"], r["type"], r["variant"]))
    built = {(r["N"], r["type"]) for r in rows if r["kind"] == "lxspec_mid"}
    routed = [(n, t) for n in factor_lengths() if n > 64 for t in ("f64", "f32") if (n, t) not in built]
    lines = [f"# sources sha256 {sources_sha256()} ({' + '.join(SOURCES)})",
             "# long 1-D real cross-spectrum kernels, gfx950 (hipcc -O3 -Rpass-analysis=kernel-resource-usage; tools/lxspec_resources.py)",
             "# kernel type N E variant vgpr agpr scratch_bytes_per_lane static_lds_bytes waves_per_simd (dynamic LDS: LxspecColsGeom, LxspecMidGeom;"
             " variant of lxspec_a: vec = two reals per access, real = one)",
             "# composed-route (N2, type): " + (", ".join(f"({n}, {t})" for n, t in routed) if routed else "none")]
    for r in rows:
        lines.append(f"{r['kind']}_kernel {r['type']} N={r['N']} E={r['E']} variant={r['variant']} vgpr={r.get('vgpr')} agpr={r.get('agpr')} "
                     f"scratch={r.get('scratch')} lds={r.get('lds')} occ={r.get('occ')}")
    spill = [r for r in rows if r.get("scratch")]
    lines.append(f"# {len(rows)} kernels, {len(spill)} with scratch: " +
                 ", ".join(f"{r['kind']} {r['type']} N={r['N']} {r['variant']} ({r['scratch']} B)" for r in spill))
    text = "\n".join(lines) + "\n"
    if args:
        Path(args[0]).parent.mkdir(parents=True, exist_ok=True)
        Path(args[0]).write_text(text)
    print(text, end="")


if __name__ == "__main__":
    main()
