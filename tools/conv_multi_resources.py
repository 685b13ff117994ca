"""Register / scratch / LDS / occupancy of the multi-output spectral-filter plans' X stage (csrc/dfft_conv_multi.hip): the fused
xconv_multi_cols_kernel of every instantiation group and the factor multiply of the dispatcher unit, from the compiler's
-Rpass-analysis=kernel-resource-usage remarks (no GPU needed).  The first line carries the sha256 of dfft_conv_multi.hip and
dfft_conv_multi.h, so tests/test_conv_multi_host.py can tell whether the inventory belongs to the sources in the tree.

  python tools/conv_multi_resources.py [out.txt]        one line per kernel, sorted by length"""
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
SOURCES = ("dfft_conv_multi.hip", "dfft_conv_multi.h", "dfft_conv_impl.h")


def sources_sha256():
    h = hashlib.sha256()
    for name in SOURCES:
        h.update((CSRC / name).read_bytes())
    return h.hexdigest()


def group_rows(g):
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{ROOT / 'include'}", f"-I{CSRC}",
           f"-DDFFT_INST_GROUP={g}", "-Rpass-analysis=kernel-resource-usage", "-c", str(CSRC / "dfft_conv_multi.hip"), "-o", "/dev/null"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-3000:])
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (.*?) \[-Rpass", line)
        if not m:
            continue
        text = m.group(1).strip()
        # xconv_multi_cols_kernel<V, Plan<N, E, ...>, REAL>: V = double2 (HIP_vector_type<double, 2>) or cpair (fp32 column pairs)
        f = re.match(r"Function Name: _ZN4dfft23xconv_multi_cols_kernelI(15HIP_vector_typeIdLj2EE|NS_5cpairE)NS_4PlanILi(\d+)ELi(\d+)E.*?ELb([01])EEEv", text)
        if f:
            cur = {"kind": "xconv_multi_cols", "type": "f64" if f.group(1).startswith("15") else "f32pair", "N": int(f.group(2)),
                   "E": int(f.group(3)), "filter": "real" if f.group(4) == "1" else "complex"}
            rows.append(cur)
            continue
        f = re.match(r"Function Name: _ZN4dfft\S*?23xconv_factor_mul_kernelI(\S*)", text)
        if f:  # <double2, double2, 1> or <f32x4, float2, 2>: 16 bytes of the slab per thread and step
            cur = {"kind": "xconv_factor_mul", "type": "f32x2" if f.group(1).startswith("Dv4_f") else "f64", "N": 0, "E": 0, "filter": "-"}
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
    rows.sort(key=lambda r: (r["N"], r["kind"], r["type"], r["filter"]))
    lines = [f"# sources sha256 {sources_sha256()} ({' + '.join(SOURCES)})",
             "# X stage of the multi-output spectral-filter plans, gfx950 (hipcc -O3 -Rpass-analysis=kernel-resource-usage; tools/conv_multi_resources.py)",
             "# kernel type N E filter vgpr agpr scratch_bytes_per_lane static_lds_bytes waves_per_simd (fused kernels: dynamic LDS, see XcGeom)"]
    for r in rows:
        lines.append(f"{r['kind']}_kernel {r['type']} N={r['N']} E={r['E']} filter={r['filter']} vgpr={r.get('vgpr')} "
                     f"agpr={r.get('agpr')} scratch={r.get('scratch')} lds={r.get('lds')} occ={r.get('occ')}")
    spill = [r for r in rows if r.get("scratch")]
    lines.append(f"# {len(rows)} kernels, {len(spill)} with scratch: " +
                 ", ".join(f"{r['kind']} {r['type']} N={r['N']} {r['filter']} ({r['scratch']} B)" for r in spill))
    text = "\n".join(lines) + "\n"
    if len(sys.argv) > 1:
        Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
        Path(sys.argv[1]).write_text(text)
    print(text, end="")


if __name__ == "__main__":
    main()
