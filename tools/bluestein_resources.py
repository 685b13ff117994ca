"""Register / scratch / occupancy of the fused Bluestein kernels (csrc/dfft_bluestein.hip), from the compiler's
-Rpass-analysis=kernel-resource-usage remarks (no GPU needed).

  python tools/bluestein_resources.py [out.txt]        every instantiation group; one line per kernel, sorted by padded length M"""
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "distributedfft_amd" / "csrc"
GROUPS = 12


def group_rows(g):
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{ROOT / 'include'}", f"-I{CSRC}",
           f"-DDFFT_INST_GROUP={g}", "-Rpass-analysis=kernel-resource-usage", "-c", str(CSRC / "dfft_bluestein.hip"), "-o", "/dev/null"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-3000:])
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (.*?) \[-Rpass", line)
        if not m:
            continue
        text = m.group(1).strip()
        f = re.match(r"Function Name: _ZN4dfft21bluestein_(rows|cols)_kernelI15HIP_vector_typeI(d|f)Lj2EENS_4PlanILi(\d+)ELi(\d+)E", text)
        if f:
            cur = {"kind": f.group(1), "type": "f64" if f.group(2) == "d" else "f32", "M": int(f.group(3)), "E": int(f.group(4))}
            rows.append(cur)
            continue
        if text.startswith("Function Name:"):
            cur = None
            continue
        if cur is None:
            continue
        for key, pat in (("vgpr", r"^VGPRs: (\d+)"), ("agpr", r"^AGPRs: (\d+)"), ("scratch", r"^ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occ", r"^Occupancy \[waves/SIMD\]: (\d+)")):
            mm = re.match(pat, text)
            if mm:
                cur[key] = int(mm.group(1))
    return rows


def main():
    with ThreadPoolExecutor(max_workers=GROUPS) as ex:
        rows = [r for rs in ex.map(group_rows, range(GROUPS)) for r in rs]
    rows.sort(key=lambda r: (r["M"], r["kind"], r["type"]))
    lines = ["# fused Bluestein kernels, gfx950 (hipcc -O3 -Rpass-analysis=kernel-resource-usage; tools/bluestein_resources.py)",
             "# kernel type M E vgpr agpr scratch_bytes_per_lane waves_per_simd"]
    for r in rows:
        lines.append(f"bluestein_{r['kind']}_kernel {r['type']} M={r['M']} E={r['E']} vgpr={r.get('vgpr')} agpr={r.get('agpr')} "
                     f"scratch={r.get('scratch')} occ={r.get('occ')}")
    spill = [r for r in rows if r.get("scratch")]
    lines.append(f"# {len(rows)} kernels, {len(spill)} with scratch: " +
                 ", ".join(f"{r['kind']} {r['type']} M={r['M']} ({r['scratch']} B)" for r in spill))
    text = "\n".join(lines) + "\n"
    if len(sys.argv) > 1:
        Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
        Path(sys.argv[1]).write_text(text)
    print(text, end="")


if __name__ == "__main__":
    main()
