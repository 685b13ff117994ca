"""Register / scratch / LDS / occupancy of the real transforms along a strided axis (csrc/dfft_real_cols.hip): the fused column-pair
kernels of every instantiation group and the pack / split / merge / unpack kernels of the dispatcher unit, from the compiler's
-Rpass-analysis=kernel-resource-usage remarks (no GPU needed).  The first line carries the sha256 of dfft_real_cols.hip and
dfft_real_cols.h, so tests/test_real_strided_host.py can tell whether the inventory belongs to the sources in the tree.

  python tools/real_cols_resources.py [out.txt]        one line per kernel, sorted by length"""
import hashlib
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from distributedfft_amd.build import NUM_INST_GROUPS as GROUPS  # noqa: E402

CSRC = ROOT / "distributedfft_amd" / "csrc"
SOURCES = ("dfft_real_cols.hip", "dfft_real_cols.h")


def sources_sha256():
    h = hashlib.sha256()
    for name in SOURCES:
        h.update((CSRC / name).read_bytes())
    return h.hexdigest()


def group_rows(g):
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{ROOT / 'include'}", f"-I{CSRC}",
           f"-DDFFT_INST_GROUP={g}", "-Rpass-analysis=kernel-resource-usage", "-c", str(CSRC / "dfft_real_cols.hip"), "-o", "/dev/null"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-3000:])
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (.*?) \[-Rpass", line)
        if not m:
            continue
        text = m.group(1).strip()
        f = re.match(r"Function Name: _ZN4dfft20(r2c|c2r)_pair_cols_kernelI15HIP_vector_typeI(d|f)Lj2EENS_4PlanILi(\d+)ELi(\d+)E.*?ELb([01])EEEv",
                     text)
        if f:
            cur = {"kind": f.group(1) + "_pair_cols", "type": "f64" if f.group(2) == "d" else "f32", "M": int(f.group(3)),
                   "E": int(f.group(4)), "vec": int(f.group(5))}
            rows.append(cur)
            continue
        f = re.match(r"Function Name: _ZN4dfft\d+(r2c_cols_pack|r2c_cols_split|c2r_cols_merge|c2r_cols_unpack)_kernelI15HIP_vector_typeI(d|f)Lj2EEEEv",
                     text)
        if f:
            cur = {"kind": f.group(1), "type": "f64" if f.group(2) == "d" else "f32", "M": 0, "E": 0, "vec": 0}
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
    with ThreadPoolExecutor(max_workers=GROUPS + 1) as ex:
        rows = [r for rs in ex.map(group_rows, range(GROUPS + 1)) for r in rs]
    rows.sort(key=lambda r: (r["M"], r["kind"], r["type"], r["vec"]))
    lines = [f"# sources sha256 {sources_sha256()} ({' + '.join(SOURCES)})",
             "# real column-pair kernels, gfx950 (hipcc -O3 -Rpass-analysis=kernel-resource-usage; tools/real_cols_resources.py)",
             "# kernel type N E vec vgpr agpr scratch_bytes_per_lane static_lds_bytes waves_per_simd (fused kernels: dynamic LDS, see ColsGeom;"
             " vec=1: column pairs loaded / stored as complex values)"]
    for r in rows:
        lines.append(f"{r['kind']}_kernel {r['type']} N={r['M']} E={r['E']} vec={r['vec']} vgpr={r.get('vgpr')} agpr={r.get('agpr')} "
                     f"scratch={r.get('scratch')} lds={r.get('lds')} occ={r.get('occ')}")
    spill = [r for r in rows if r.get("scratch")]
    lines.append(f"# {len(rows)} kernels, {len(spill)} with scratch: " +
                 ", ".join(f"{r['kind']} {r['type']} N={r['M']} vec={r['vec']} ({r['scratch']} B)" for r in spill))
    text = "\n".join(lines) + "\n"
    if len(sys.argv) > 1:
        Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
        Path(sys.argv[1]).write_text(text)
    print(text, end="")


if __name__ == "__main__":
    main()
