"""Register / scratch / LDS / occupancy of the kernels the real-field spectral-filter plans add (csrc/dfft_conv_real.hip: the filter
re-layout), from the compiler's -Rpass-analysis=kernel-resource-usage remarks (no GPU needed).  The first line carries the sha256 of
dfft_conv_real.hip and dfft_conv_real.h, so tests/test_conv_real_host.py can tell whether the inventory belongs to the sources in the tree.
(The X stage these plans run is dfft_conv.hip's: tools/conv_resources.py, profiles/r12/kernel_resources.txt.)

  python tools/conv_real_resources.py [out.txt]        one line per kernel"""
import hashlib
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "distributedfft_amd" / "csrc"
SOURCES = ("dfft_conv_real.hip", "dfft_conv_real.h")
# mangled element type of xconv_real_relayout_kernel<E> -> what the inventory calls it
TYPES = {"d": "f64-real", "f": "f32-real", "15HIP_vector_typeIdLj2EE": "f64-complex", "15HIP_vector_typeIfLj2EE": "f32-complex"}


def sources_sha256():
    h = hashlib.sha256()
    for name in SOURCES:
        h.update((CSRC / name).read_bytes())
    return h.hexdigest()


def rows():
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{ROOT / 'include'}", f"-I{CSRC}",
           "-Rpass-analysis=kernel-resource-usage", "-c", str(CSRC / "dfft_conv_real.hip"), "-o", "/dev/null"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-3000:])
    out, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (.*?) \[-Rpass", line)
        if not m:
            continue
        text = m.group(1).strip()
        f = re.match(r"Function Name: _ZN4dfft\S*?26xconv_real_relayout_kernelI(\S+?)EEvPKT_", text)
        if f:
            cur = {"kind": "xconv_real_relayout", "type": TYPES.get(f.group(1), f.group(1))}
            out.append(cur)
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
    return sorted(out, key=lambda r: r["type"])


def main():
    rs = rows()
    lines = [f"# sources sha256 {sources_sha256()} ({' + '.join(SOURCES)})",
             "# kernels of the real-field spectral-filter plans, gfx950 (hipcc -O3 -Rpass-analysis=kernel-resource-usage; tools/conv_real_resources.py)",
             "# kernel type vgpr agpr scratch_bytes_per_lane static_lds_bytes waves_per_simd"]
    for r in rs:
        lines.append(f"{r['kind']}_kernel {r['type']} vgpr={r.get('vgpr')} agpr={r.get('agpr')} scratch={r.get('scratch')} lds={r.get('lds')} "
                     f"occ={r.get('occ')}")
    spill = [r for r in rs if r.get("scratch")]
    lines.append(f"# {len(rs)} kernels, {len(spill)} with scratch")
    text = "\n".join(lines) + "\n"
    if len(sys.argv) > 1:
        Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
        Path(sys.argv[1]).write_text(text)
    print(text, end="")


if __name__ == "__main__":
    main()
