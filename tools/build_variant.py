"""Developer helper: a second build of the library with extra compile-time switches on the FFT kernel units, dfft_zy.hip and the host units that
include dfft_zy.h, for A/B runs on the GPU box (DFFT_LIB=<path> selects it in the Python harness).   python tools/build_variant.py <name> -DSWITCH=value ...
-> distributedfft_amd/lib/libdfft_variant_<name>.so (linked against the HIP / RCCL runtime bundled with PyTorch)."""
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from distributedfft_amd import build as B  # noqa: E402

name, flags = sys.argv[1], sys.argv[2:]
B.build()
obj = B.LIBDIR / f"obj_variant_{name}"
obj.mkdir(parents=True, exist_ok=True)
units = [(B.CSRC / "dfft_fft_inst.hip", obj / f"dfft_fft_inst_{g}.o", [f"-DDFFT_INST_GROUP={g}"] + flags) for g in range(B.NUM_INST_GROUPS)]
units.append((B.CSRC / "dfft_zy.hip", obj / "dfft_zy.o", flags))  # the one-launch YZ stage has build-time switches of its own
# ... which the plan may have to know (a switch that changes ZyLaunch): every host unit that includes dfft_zy.h
zy_h = (B.CSRC / "dfft_zy.h").resolve()
units += [(B.CSRC / f"{n}.cpp", obj / f"{n}.o", ["-x", "hip"] + flags) for n in B.HOST_UNITS if zy_h in B._deps(B.CSRC / f"{n}.cpp")]
with ThreadPoolExecutor(max_workers=8) as ex:
    list(ex.map(lambda u: B._run([B.HIPCC] + B.COMMON + u[2] + ["-c", str(u[0]), "-o", str(u[1])]), units))
# everything else as the regular build made it
rebuilt = {u[1].name for u in units}
others = [str(o) for _, o, _ in B.units() if o.name not in rebuilt]
tl = B._torch_lib_dir()
out = B.LIBDIR / f"libdfft_variant_{name}.so"
B._run(["g++", "-shared", "-fPIC", "-o", str(out)] + [str(u[1]) for u in units] + others +
       ["-L" + str(tl), "-l:libamdhip64.so", "-l:librccl.so", "-lpthread", "-Wl,-rpath," + str(tl)])
print(out)
