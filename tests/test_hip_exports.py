"""Every entry point registered in the HIP kernel library (``_hip``) is reachable from the
package or from a product test: a kernel nobody calls is pruned, not shipped (diagnostic
variants live in git history and their results in ``profiles/``).  Host logic, no GPU."""
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_every_hip_export_has_a_caller():
    from flink_tensorflow_amd import _ext

    hip = _ext.hip(required=False)
    if hip is None:
        pytest.skip("HIP kernel library not built")
    exports = sorted(n for n in dir(hip) if not n.startswith("_") and callable(getattr(hip, n)))
    assert exports, "the kernel library registers no entry point"
    here = Path(__file__).resolve()
    text = "\n".join(p.read_text(errors="replace")
                     for d in ("flink_tensorflow_amd", "tests") for p in sorted((ROOT / d).rglob("*.py"))
                     if p.resolve() != here)
    words = set(re.findall(r"\w+", text))
    orphans = [n for n in exports if n not in words]
    assert not orphans, f"_hip entry points without a caller in the package or the tests: {orphans}"
