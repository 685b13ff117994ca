"""Register / scratch / LDS / occupancy inventories of the fused 1-D real kernel families, from the compiler's
-Rpass-analysis=kernel-resource-usage remarks (no GPU needed): one table entry per family, one inventory per family under profiles/.

  python tools/fused_resources.py <family> [out.txt]     print the family's inventory (and write it to out.txt)
  python tools/fused_resources.py --all                   rewrite the committed inventory of every family
  python tools/fused_resources.py lxspec --build-all      ... with lxspec_fused_ok overridden to build every Mid kernel (to find the spilling ones)
  ... --asm-dir DIR                                       keep each group's device assembly in DIR (the input of tools/kernel_isa_diff.py)

The first line of an inventory carries the sha256 of the family's .hip and of every project header it includes, transitively, so the
host tests (tests/test_*_host.py) can tell whether the inventory belongs to the sources in the tree."""
import argparse
import hashlib
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from distributedfft_amd.build import ARCH, HIPCC, NUM_INST_GROUPS as GROUPS, _deps  # noqa: E402

CSRC = ROOT / "distributedfft_amd" / "csrc"
KEYS = (("vgpr", r"^VGPRs: (\d+)"), ("agpr", r"^AGPRs: (\d+)"), ("scratch", r"^ScratchSize \[bytes/lane\]: (\d+)"),
        ("lds", r"^LDS Size \[bytes/block\]: (\d+)"), ("occ", r"^Occupancy \[waves/SIMD\]: (\d+)"))
PLAN = r"I15HIP_vector_typeI(d|f)Lj2EENS_4PlanILi(\d+)ELi(\d+)E"   # <V, Plan<N, E, ...>: groups type, length, E
TYPES = ("f64", "f32")


def tuned_lengths():
    return sorted({int(n) for n in re.findall(r"^\s*X\((\d+),", (CSRC / "dfft_plans.h").read_text(), re.M)})


def factor_lengths():
    return sorted({b << a for b in (1, 3, 5) for a in range(12) if 64 <= b << a <= 2048} | {81, 125})


def _ftype(args):       # precision of an element-wise kernel from its mangled template arguments
    return "f64" if (args.startswith("d") or "HIP_vector_typeIdLj2E" in args) else "f32"


def _hkind(args):       # element type of the filter of a *_mul kernel
    return "complex" if args.count("HIP_vector_type") == 2 or args.endswith("S2_") else "real"


# A family: the source unit; the committed inventory; `length`, the name of the length column; `fields`, the columns between E and vgpr;
# `fused`: (kernel name, tail of the pattern behind the plan, function of the tail's groups -> fields); `plain`: the element-wise kernels
# of the dispatcher unit and a function (name, template arguments) -> fields; `routed`: label and function (rows) -> the instantiations
# that run the composed route; `title` / `columns`: lines 2 and 3.  The sort key is (length, kernel, type, fields...).
def _any(fields):
    return lambda name, a: {f: "any" for f in fields}


FAMILIES = {
    "rconv": dict(
        unit="dfft_rconv.hip", inventory="profiles/2026-10-19_rconv1d/kernel_resources.txt", length="M", fields=("filter", "form"),
        title="1-D real FFT convolution kernels, gfx950 (hipcc -O3 -Rpass-analysis=kernel-resource-usage; tools/rconv_resources.py)",
        columns="(fused kernel: dynamic LDS, see RconvGeom; form vec: two reals per access, real: one)",
        fused=(("rconv_rows", r".*?EELb([01])ELb([01])EEEv", lambda h, v: {"filter": "real" if h == "1" else "complex", "form": "vec" if v == "1" else "real"}),),
        plain=(("rconv_mul",), lambda name, a: {"filter": _hkind(a), "form": "any"}),
        routed=("composed-route (M, type, filter, form)",
                lambda built: [(n, t, f, a) for n in tuned_lengths() for t in TYPES for f in ("complex", "real") for a in ("vec", "real")
                               if (n, t, f, a) not in built])),
    "osconv": dict(
        unit="dfft_osconv.hip", inventory="profiles/2026-10-20_rconv1d_os/kernel_resources.txt", length="M", fields=("filter", "form"),
        title="overlap-save 1-D real FFT convolution kernels, gfx950 (hipcc -O3 -Rpass-analysis=kernel-resource-usage; tools/osconv_resources.py)",
        columns="(block kernel: dynamic LDS, see RconvGeom; form vec: two reals per access, real: one)",
        fused=(("osconv_blocks", r".*?EELb([01])ELb([01])EEEv", lambda h, v: {"filter": "real" if h == "1" else "complex", "form": "vec" if v == "1" else "real"}),),
        plain=(("osconv_gather", "osconv_scatter", "osconv_mul"), lambda name, a: {"filter": _hkind(a) if name == "osconv_mul" else "any", "form": "any"}),
        routed=("composed-route (M, type, filter, form)",
                lambda built: [(n, t, f, a) for n in tuned_lengths() for t in TYPES for f in ("complex", "real") for a in ("vec", "real")
                               if (n, t, f, a) not in built])),
    "lconv": dict(
        unit="dfft_lconv.hip", inventory="profiles/2026-10-20_rconv1d_long/kernel_resources.txt", length="N", fields=("variant",),
        title="long 1-D real FFT convolution kernels, gfx950 (hipcc -O3 -Rpass-analysis=kernel-resource-usage; tools/lconv_resources.py)",
        columns="(dynamic LDS: LconvColsGeom, LconvMidGeom; variant of lconv_a / lconv_c: vec = two reals per access, real = one; of lconv_mid: the filter's"
                " element type)",
        fused=(("lconv_a", r".*?EELb([01])EEEv", lambda v: {"variant": "vec" if v == "1" else "real"}),
               ("lconv_c", r".*?EELb([01])EEEv", lambda v: {"variant": "vec" if v == "1" else "real"}),
               ("lconv_mid", r".*?EELb([01])EEEv", lambda h: {"variant": "real" if h == "1" else "complex"})),
        plain=(("lconv_filter", "lconv_mul"),
               lambda name, a: {"variant": _hkind(a) if name == "lconv_mul" else "16B" if "HIP_vector_type" in a else "8B" if a.startswith("d") else "4B"}),
        routed=("composed-route (N, type)", lambda built: [(n, t) for n in factor_lengths() for t in TYPES if (n, t) not in {b[:2] for b in built}])),
    "stft": dict(
        unit="dfft_stft.hip", inventory="profiles/2026-10-20_stft/kernel_resources.txt", length="M", fields=("out", "form"),
        title="short-time Fourier transform kernels, gfx950 (hipcc -O3 -Rpass-analysis=kernel-resource-usage; tools/stft_resources.py)",
        columns="(frame kernel: dynamic LDS, see RconvGeom; form vec: whole frames two reals per access, real: one)",
        fused=(("stft_frames", r".*?EELb([01])ELb([01])EEEv", lambda p, v: {"out": "power" if p == "1" else "complex", "form": "vec" if v == "1" else "real"}),),
        plain=(("stft_gather", "stft_power", "istft_ola"), _any(("out", "form"))),
        routed=("composed-route (M, type, out, form), stft_fused_ok",
                lambda built: [(n, t, o, a) for n in tuned_lengths() for t in TYPES for o in ("complex", "power") for a in ("vec", "real")
                               if (n, t, o, a) not in built])),
    "rxspec": dict(
        unit="dfft_xspec.hip", inventory="profiles/2026-10-20_rxspec1d/kernel_resources.txt", length="M", fields=("form",),
        title="1-D real cross-spectrum kernels, gfx950 (hipcc -O3 -Rpass-analysis=kernel-resource-usage; tools/rxspec_resources.py)",
        columns="(fused kernel: dynamic LDS, see RconvGeom; form vec: two reals per access, real: one)",
        fused=(("rxspec_rows", r".*?EELb([01])EEEv", lambda v: {"form": "vec" if v == "1" else "real"}),),
        plain=(("rxspec_mac",), _any(("form",))),
        routed=("composed-route (M, type, form)",
                lambda built: [(n, t, a) for n in tuned_lengths() for t in TYPES for a in ("vec", "real") if (n, t, a) not in built])),
    "lxspec": dict(
        unit="dfft_lxspec.hip", inventory="profiles/2026-10-20_rxspec1d_long/kernel_resources.txt", length="N", fields=("variant",),
        title="long 1-D real cross-spectrum kernels, gfx950 (hipcc -O3 -Rpass-analysis=kernel-resource-usage; tools/lxspec_resources.py)",
        columns="(dynamic LDS: LxspecColsGeom, LxspecMidGeom; variant of lxspec_a: vec = two reals per access, real = one)",
        fused=(("lxspec_a", r".*?EELb([01])EEEv", lambda v: {"variant": "vec" if v == "1" else "real"}),
               ("lxspec_mid", r"", lambda: {"variant": "any"})),
        plain=(("lxspec_reduce", "lxspec_mac"), _any(("variant",))),
        routed=("composed-route (N2, type)", None)),   # the Mid kernels decide: routed_of
    "rcsd": dict(
        unit="dfft_csd.hip", inventory="profiles/2026-10-20_rcsd1d/kernel_resources.txt", length="M", fields=("form",),
        title="framed 1-D real cross-spectrum kernels, gfx950 (hipcc -O3 -Rpass-analysis=kernel-resource-usage; tools/rcsd_resources.py)",
        columns="(fused kernel: dynamic LDS, see RconvGeom; form vec: two reals per access, real: one)",
        fused=(("rcsd_frames", r".*?EELb([01])ELb([01])EEEv", lambda v, a: {"form": ("vec" if v == "1" else "real") + ("-auto" if a == "1" else "-cross")}),),
        plain=(("rcsd_gather", "rcsd_mac"), _any(("form",))),
        routed=("composed-route (M, type, form)",
                lambda built: [(n, t, a) for n in tuned_lengths() for t in TYPES for a in ("vec-auto", "vec-cross", "real-auto", "real-cross")
                               if (n, t, a) not in built])),
    # the element-wise kernels the families share: compiled once, no instantiation groups, nothing routed
    "rows_common": dict(
        unit="dfft_rows_common.hip", inventory="profiles/2026-10-21_fused_scaffold/kernel_resources.txt", length="M", fields=("form",), groups=False,
        title="element-wise kernels shared by the 1-D real kernel families, gfx950 (hipcc -O3 -Rpass-analysis=kernel-resource-usage;"
              " tools/fused_resources.py rows_common)",
        columns="",
        fused=(), plain=(("pad_rows", "trunc_rows", "slice_reduce"), _any(("form",))),
        routed=("composed-route", lambda built: [])),
}


def sources(family):
    """The family's .hip and every project header it includes, transitively, sorted by name."""
    return sorted(_deps(CSRC / FAMILIES[family]["unit"]), key=lambda p: p.name)


def sources_sha256(family):
    h = hashlib.sha256()
    for p in sources(family):
        h.update(p.read_bytes())
    return h.hexdigest()


def group_rows(family, g, extra=(), asm_dir=None):
    F = FAMILIES[family]
    src = CSRC / F["unit"]
    out = ["-c", "-o", "/dev/null"]
    if asm_dir is not None:   # the flags of the library build minus compression, device side only
        out = ["--cuda-device-only", "-S", "-o", str(Path(asm_dir) / (src.stem + ("" if g is None else f"_{g}") + ".s"))]
    cmd = [HIPCC, "--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", f"-I{ROOT / 'include'}", f"-I{CSRC}", *extra,
           *([] if g is None else [f"-DDFFT_INST_GROUP={g}"]), "-Rpass-analysis=kernel-resource-usage", *out[:-2], str(src), *out[-2:]]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-3000:])
    L = F["length"]
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (.*?) \[-Rpass", line)
        if not m:
            continue
        text = m.group(1).strip()
        if text.startswith("Function Name:"):
            cur = None
            for name, tail, fields in F["fused"]:
                f = re.match(r"Function Name: _ZN4dfft\d+" + name + "_kernel" + PLAN + tail, text)
                if f:
                    cur = {"kind": name, "type": "f64" if f.group(1) == "d" else "f32", L: int(f.group(2)), "E": int(f.group(3)), **fields(*f.groups()[3:])}
            f = re.match(r"Function Name: _ZN4dfft\d+(" + "|".join(F["plain"][0]) + r")_kernelI(.*)EEv", text)
            if f:
                cur = {"kind": f.group(1), "type": _ftype(f.group(2)), L: 0, "E": 0, **F["plain"][1](f.group(1), f.group(2))}
            if cur is not None:
                rows.append(cur)
            continue
        if cur is None:
            continue
        for key, pat in KEYS:
            mm = re.match(pat, text)
            if mm:
                cur[key] = int(mm.group(1))
    return rows


def routed_of(family, rows):
    F = FAMILIES[family]
    L = F["length"]
    if family == "lxspec":   # pass A of every factor length is built: the Mid kernel of the longer factor decides
        built = {(r[L], r["type"]) for r in rows if r["kind"] == "lxspec_mid"}
        return [(n, t) for n in factor_lengths() if n > 64 for t in TYPES if (n, t) not in built]
    return F["routed"][1]({(r[L], r["type"], *(r[f] for f in F["fields"])) for r in rows if r[L]})


def inventory(family, extra=(), asm_dir=None):
    F = FAMILIES[family]
    L, fields = F["length"], F["fields"]
    groups = list(range(GROUPS + 1)) if F.get("groups", True) else [None]
    with ThreadPoolExecutor(max_workers=min(len(groups), os.cpu_count() or 4, 16)) as ex:
        rows = [r for rs in ex.map(lambda g: group_rows(family, g, extra, asm_dir), groups) for r in rs]
    rows.sort(key=lambda r: (r[L], r["kind"], r["type"], *(r[f] for f in fields)))
    routed = routed_of(family, rows)
    names = [p.name for p in sources(family)]
    cols = " ".join(fields)
    lines = [f"# sources sha256 {sources_sha256(family)} ({' + '.join(names)})",
             "# " + F["title"],
             f"# kernel type {L} E {cols} vgpr agpr scratch_bytes_per_lane static_lds_bytes waves_per_simd" + (" " + F["columns"] if F["columns"] else ""),
             f"# {F['routed'][0]}: " + (", ".join("(" + ", ".join(str(x) for x in t) + ")" for t in routed) if routed else "none")]
    for r in rows:
        lines.append(f"{r['kind']}_kernel {r['type']} {L}={r[L]} E={r['E']} " + " ".join(f"{f}={r[f]}" for f in fields) +
                     f" vgpr={r.get('vgpr')} agpr={r.get('agpr')} scratch={r.get('scratch')} lds={r.get('lds')} occ={r.get('occ')}")
    spill = [r for r in rows if r.get("scratch")]
    lines.append(f"# {len(rows)} kernels, {len(spill)} with scratch: " +
                 ", ".join(f"{r['kind']} {r['type']} {L}={r[L]} " + " ".join(str(r[f]) for f in fields) + f" ({r['scratch']} B)" for r in spill))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("family", nargs="?", choices=sorted(FAMILIES))
    ap.add_argument("out", nargs="?")
    ap.add_argument("--all", action="store_true", help="rewrite the committed inventory of every family")
    ap.add_argument("--build-all", action="store_true", help="lxspec: build every Mid kernel")
    ap.add_argument("--asm-dir", help="keep each group's device assembly here")
    a = ap.parse_args()
    if a.all == bool(a.family):
        ap.error("give one family, or --all")
    if a.asm_dir:
        Path(a.asm_dir).mkdir(parents=True, exist_ok=True)
    for family in (sorted(FAMILIES) if a.all else [a.family]):
        text = inventory(family, ("-DDFFT_LXSPEC_BUILD_ALL",) if a.build_all and family == "lxspec" else (), a.asm_dir)
        out = ROOT / FAMILIES[family]["inventory"] if a.all else a.out
        if out:
            Path(out).parent.mkdir(parents=True, exist_ok=True)
            Path(out).write_text(text)
        if not a.all:
            print(text, end="")


if __name__ == "__main__":
    main()
