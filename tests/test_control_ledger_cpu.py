"""CPU: the kernel ledger for lightdiffusion_amd/csrc/control/.  tests/test_errbound_cpu.py::test_every_norm_and_misc_kernel_is_held_by_a_gpu_test
enumerates the translation units directly under csrc; this restates its rule for the units of the subdirectory, with its pattern, as
tests/test_regional_ledger_cpu.py does for csrc/regional/: every __global__ *_kernel found there has a row in
tests/test_control_ops_gpu.py::KERNELS that names callable tests of that module, and no row names a kernel that no longer exists."""
import importlib
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import ROOT                     # noqa: E402
from test_errbound_cpu import KERNEL_PAT      # noqa: E402

CONTROL = os.path.join(ROOT, "lightdiffusion_amd", "csrc", "control")
HOLDER = "test_control_ops_gpu"


def control_kernels():
    found = {}
    for dp, _, files in os.walk(CONTROL):
        for f in sorted(files):
            if f.endswith((".hip", ".h")):
                for k in re.findall(KERNEL_PAT, open(os.path.join(dp, f)).read()):
                    found.setdefault(k, []).append(os.path.relpath(os.path.join(dp, f), CONTROL))
    return found


def test_every_control_kernel_is_held_by_a_gpu_test():
    kernels = control_kernels()
    assert set(kernels) >= {"control_add_kernel", "hint_conv_kernel"}, "the pattern or the directory moved"
    assert all(len(v) == 1 for v in kernels.values()), f"a kernel name defined twice: {kernels}"
    mod = importlib.import_module(HOLDER)
    assert mod.KERNELS, f"{HOLDER}.KERNELS is empty"
    assert getattr(mod.pytestmark, "name", None) == "gpu", f"{HOLDER} must be marked gpu as a whole"
    for k, tests in mod.KERNELS.items():
        assert tests and all(t.startswith("test_") and callable(getattr(mod, t, None)) for t in tests), (HOLDER, k, tests)
    missing = set(kernels) - set(mod.KERNELS)
    assert not missing, f"csrc/control: kernels without a bitwise or element-wise GPU test: {sorted(missing)}"
    gone = set(mod.KERNELS) - set(kernels)
    assert not gone, f"{HOLDER}: rows for kernels that no longer exist: {sorted(gone)}"


def test_control_kernels_do_not_shadow_the_other_ledgers():
    """The names are new: none of them is a kernel of a unit another ledger enumerates."""
    csrc = os.path.dirname(CONTROL)
    other = set()
    for dp, _, files in os.walk(csrc):
        if os.path.abspath(dp) == os.path.abspath(CONTROL) or os.path.basename(dp) == "build" or os.sep + "build" + os.sep in dp + os.sep:
            continue
        for f in files:
            if f.endswith((".hip", ".h")):
                other |= set(re.findall(KERNEL_PAT, open(os.path.join(dp, f)).read()))
    assert other and not other & set(control_kernels())


def test_the_unit_is_built_without_contraction_in_both_trees():
    """the control add is held bitwise to its expression: the Makefile gives the unit -ffp-contract=off in the product and the A/B build"""
    mk = open(os.path.join(ROOT, "lightdiffusion_amd", "csrc", "Makefile")).read()
    assert "control/control.hip" in re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1)
    assert re.search(r"^build/control/control\.o build/ab_control/control\.o: CXXFLAGS \+= -ffp-contract=off$", mk, re.M)
