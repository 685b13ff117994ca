"""Register / scratch / LDS / occupancy of the framed (Welch) 1-D real cross-spectrum (csrc/dfft_csd.hip): the fused kernel of every
instantiation group (tuned half-length M x fp64 / fp32 x two-real / per-real accesses) and the reduce, gather and multiply-accumulate
kernels of the dispatcher unit, from the compiler's -Rpass-analysis=kernel-resource-usage remarks (no GPU needed).  The first line
carries the sha256 of dfft_csd.hip and dfft_csd.h, so tests/test_rcsd1d_host.py can tell whether the inventory belongs to the
sources in the tree.

  python tools/rcsd_resources.py [out.txt]        one line per kernel, sorted by length"""
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
SOURCES = ("dfft_csd.hip", "dfft_csd.h")
FORMS = ("vec-auto", "vec-cross", "real-auto", "real-cross")   # two-real values / per-real accesses x auto- / cross-spectrum kernel


def sources_sha256():
    h = hashlib.sha256()
    for name in SOURCES:
        h.update((CSRC / name).read_bytes())
    return h.hexdigest()


def tuned_lengths():
    return sorted({int(n) for n in re.findall(r"^\s*X\((\d+),", (CSRC / "dfft_plans.h").read_text(), re.M)})


def group_rows(g):
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{ROOT / 'include'}", f"-I{CSRC}",
           f"-DDFFT_INST_GROUP={g}", "-Rpass-analysis=kernel-resource-usage", "-c", str(CSRC / "dfft_csd.hip"), "-o", "/dev/null"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-3000:])
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (.*?) \[-Rpass", line)
        if not m:
            continue
        text = m.group(1).strip()
        f = re.match(r"Function Name: _ZN4dfft18rcsd_frames_kernelI15HIP_vector_typeI(d|f)Lj2EENS_4PlanILi(\d+)ELi(\d+)E.*?EELb([01])ELb([01])EEEv", text)
        if f:
            cur = {"kind": "rcsd_frames", "type": "f64" if f.group(1) == "d" else "f32", "M": int(f.group(2)), "E": int(f.group(3)),
                   "form": ("vec" if f.group(4) == "1" else "real") + ("-auto" if f.group(5) == "1" else "-cross")}
            rows.append(cur)
            continue
        f = re.match(r"Function Name: _ZN4dfft\d+(rcsd_reduce|rcsd_gather|rcsd_mac)_kernelI(.*)EEv", text)
        if f:
            a = f.group(2)
            cur = {"kind": f.group(1), "type": "f64" if (a.startswith("d") or "HIP_vector_typeIdLj2E" in a) else "f32", "M": 0, "E": 0, "form": "any"}
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
    with ThreadPoolExecutor(max_workers=min(GROUPS + 1, os.cpu_count() or 4, 16)) as ex:
        rows = [r for rs in ex.map(group_rows, range(GROUPS + 1)) for r in rs]
    rows.sort(key=lambda r: (r["M"], r["kind"], r["type"], r["form"]))
    built = {(r["M"], r["type"], r["form"]) for r in rows if r["M"]}
    routed = [(n, t, a) for n in tuned_lengths() for t in ("f64", "f32") for a in FORMS if (n, t, a) not in built]
    lines = [f"# sources sha256 {sources_sha256()} ({' + '.join(SOURCES)})",
             "# framed 1-D real cross-spectrum kernels, gfx950 (hipcc -O3 -Rpass-analysis=kernel-resource-usage; tools/rcsd_resources.py)",
             "# kernel type M E form vgpr agpr scratch_bytes_per_lane static_lds_bytes waves_per_simd (fused kernel: dynamic LDS, see RconvGeom;"
             " form vec: two reals per access, real: one)",
             "# composed-route (M, type, form): " + (", ".join(f"({n}, {t}, {a})" for n, t, a in routed) if routed else "none")]
    for r in rows:
        lines.append(f"{r['kind']}_kernel {r['type']} M={r['M']} E={r['E']} form={r['form']} vgpr={r.get('vgpr')} agpr={r.get('agpr')} "
                     f"scratch={r.get('scratch')} lds={r.get('lds')} occ={r.get('occ')}")
    spill = [r for r in rows if r.get("scratch")]
    lines.append(f"# {len(rows)} kernels, {len(spill)} with scratch: " +
                 ", ".join(f"{r['kind']} {r['type']} M={r['M']} {r['form']} ({r['scratch']} B)" for r in spill))
    text = "\n".join(lines) + "\n"
    if len(sys.argv) > 1:
        Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
        Path(sys.argv[1]).write_text(text)
    print(text, end="")


if __name__ == "__main__":
    main()
