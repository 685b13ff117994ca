"""What the host tests of the fused 1-D real kernel families share about their committed resource inventories: the inventory tool
(tools/fused_resources.py, loaded by path), the check that an inventory belongs to the sources in the tree, and the lines of the
element-wise kernels that live in the common unit (csrc/dfft_rows_common.hip)."""
import importlib.util
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
_TOOL = []


def tool():
    if not _TOOL:
        spec = importlib.util.spec_from_file_location("fused_resources", ROOT / "tools" / "fused_resources.py")
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _TOOL.append(mod)
    return _TOOL[0]


def current_text(family):
    """The family's committed inventory, after checking that its first line carries the sha256 of the family's unit and of every
    project header the unit includes."""
    fr = tool()
    text = (ROOT / fr.FAMILIES[family]["inventory"]).read_text()
    m = re.match(r"# sources sha256 ([0-9a-f]{64}) ", text)
    assert m and m.group(1) == fr.sources_sha256(family), f"regenerate with: python tools/fused_resources.py {family} {fr.FAMILIES[family]['inventory']}"
    return text


def common_lines(*prefixes):
    """The lines of the common unit's inventory (checked against its sources) that start with one of the prefixes."""
    return [ln for ln in current_text("rows_common").splitlines() if ln.startswith(prefixes)]
