"""CPU: the kernel ledger for lightdiffusion_amd/csrc/inpaint/.  tests/test_errbound_cpu.py::test_every_norm_and_misc_kernel_is_held_by_a_gpu_test
enumerates the translation units directly under csrc; this restates its rule for the units of the subdirectory, with its pattern, as
tests/test_detail_ledger_cpu.py does for csrc/detail/: every __global__ *_kernel found there has a row in tests/test_inpaint_ops_gpu.py::KERNELS that
names callable tests of that module, and no row names a kernel that no longer exists."""
import importlib
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import ROOT                     # noqa: E402
from test_errbound_cpu import KERNEL_PAT      # noqa: E402

INPAINT = os.path.join(ROOT, "lightdiffusion_amd", "csrc", "inpaint")
HOLDER = "test_inpaint_ops_gpu"


def inpaint_kernels():
    found = {}
    for dp, _, files in os.walk(INPAINT):
        for f in sorted(files):
            if f.endswith((".hip", ".h")):
                for k in re.findall(KERNEL_PAT, open(os.path.join(dp, f)).read()):
                    found.setdefault(k, []).append(os.path.relpath(os.path.join(dp, f), INPAINT))
    return found


def test_every_inpaint_kernel_is_held_by_a_gpu_test():
    kernels = inpaint_kernels()
    assert kernels, "no kernel found under csrc/inpaint: the pattern or the directory moved"
    assert all(len(v) == 1 for v in kernels.values()), f"a kernel name defined twice: {kernels}"
    mod = importlib.import_module(HOLDER)
    assert mod.KERNELS, f"{HOLDER}.KERNELS is empty"
    assert getattr(mod.pytestmark, "name", None) == "gpu", f"{HOLDER} must be marked gpu as a whole"
    for k, tests in mod.KERNELS.items():
        assert tests and all(t.startswith("test_") and callable(getattr(mod, t, None)) for t in tests), (HOLDER, k, tests)
    missing = set(kernels) - set(mod.KERNELS)
    assert not missing, f"csrc/inpaint: kernels without a bitwise GPU test: {sorted(missing)}"
    gone = set(mod.KERNELS) - set(kernels)
    assert not gone, f"{HOLDER}: rows for kernels that no longer exist: {sorted(gone)}"


def test_inpaint_kernels_do_not_shadow_the_other_ledgers():
    """The names are new: none of them is a kernel of a unit the top-level ledger or the csrc/detail ledger enumerates (an overloaded name would be
    held there by a test that never runs it)."""
    csrc = os.path.dirname(INPAINT)
    other = set()
    for dp, _, files in os.walk(csrc):
        if os.path.abspath(dp) == os.path.abspath(INPAINT) or os.path.basename(dp) == "build" or os.sep + "build" + os.sep in dp + os.sep:
            continue
        for f in files:
            if f.endswith((".hip", ".h")):
                other |= set(re.findall(KERNEL_PAT, open(os.path.join(dp, f)).read()))
    assert other and not other & set(inpaint_kernels())
