"""Compare the device assembly of two builds kernel by kernel: a plain text diff keyed by kernel symbol.

  python tools/kernel_isa_diff.py OLD_DIR NEW_DIR [--rename OLD=NEW ...]

Both directories hold the `.s` files of `hipcc --cuda-device-only -S` (tools/fused_resources.py --asm-dir writes them, one per unit and
instantiation group).  A kernel's text runs from its label through its `.end_amdhsa_kernel`; its own symbol is replaced by a
placeholder inside that text, so a renamed kernel compares equal when nothing else changed.  --rename maps a substring of the old
kernel names to the new one (a kernel that moved to another unit under another name).  Prints one line per differing or unmatched
kernel and a summary; exit status 1 if a kernel that exists on both sides differs."""
import argparse
import re
import sys
from pathlib import Path


def kernels(directory):
    """symbol -> text of every kernel in the directory's .s files"""
    out = {}
    for path in sorted(Path(directory).glob("*.s")):
        text = path.read_text()
        for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)$", text, re.M):
            sym = m.group(1)
            start = text.rfind("\n" + sym + ":", 0, m.start())
            end = text.index(".end_amdhsa_kernel", m.end())
            if start < 0:
                raise SystemExit(f"{path}: no label for {sym}")
            body = text[start + 1:end].replace(sym, "<kernel>")
            # local labels carry the ordinal of the function in its file (.LBB3_25, BB3_5, .Lfunc_end3), and the comments behind them are
            # aligned to a column: neither is part of the kernel
            body = re.sub(r"(\.LBB|\bBB|\.Lfunc_begin|\.Lfunc_end)\d+", r"\1", body)
            out[sym] = re.sub(r"[ \t]+;", " ;", body)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    for r in a.rename:
        src, dst = r.split("=", 1)
        # mangled names carry the length of the identifier in front of it
        old = {re.sub(r"\d+" + re.escape(src), f"{len(dst)}{dst}", k) if src in k else k: v for k, v in old.items()}
    same = differ = 0
    for sym in sorted(old.keys() & new.keys()):
        if old[sym] == new[sym]:
            same += 1
        else:
            differ += 1
            print("DIFFERS", sym)
    for sym in sorted(old.keys() - new.keys()):
        print("ONLY OLD", sym)
    for sym in sorted(new.keys() - old.keys()):
        print("ONLY NEW", sym)
    print(f"{len(old)} old kernels, {len(new)} new kernels, {same + differ} compared, {differ} differing, "
          f"{len(old.keys() - new.keys())} only old, {len(new.keys() - old.keys())} only new")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
