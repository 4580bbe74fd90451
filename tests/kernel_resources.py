"""What the resource tests (tests/test_*_resources.py) share.  hipcc cross-compiles a device file for gfx950 without a GPU
and reports every kernel's resources; compiling, reading the remarks and the records under profiles/ are
tools/kernel_usage.py, which `make asm` uses too.  Here: each file compiled once per session, and the bars the tests hold."""

import functools
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import kernel_usage  # noqa: E402
from kernel_usage import HIPCC, ROOT, row  # noqa: E402,F401

# compile_kernels(name, defines=()): every kernel of cudabrot_amd/csrc/<name>.hip as the compiler reports it, a dict of its
# mangled "name" and the figures by the compiler's own labels, and the assembly it wrote; `defines` is a tuple
compile_kernels = functools.lru_cache(maxsize=None)(kernel_usage.compile_kernels)


def at_most(vgprs, waves):
    return lambda k: int(k["VGPRs"]) <= vgprs and int(k["Occupancy [waves/SIMD]"]) >= waves


def no_spill_no_scratch(k):
    return int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0 and int(k["ScratchSize [bytes/lane]"]) == 0


def matches_record(kernels, name):
    """profiles/<name>_kernel_usage.txt names these kernels and no other, each with the compiler's six figures."""
    record = kernel_usage.read_record(name)
    assert sorted(record) == sorted(k["name"] for k in kernels)
    for k in kernels:
        assert record[k["name"]] == kernel_usage.figures(k), (k["name"], record[k["name"]], kernel_usage.figures(k))


# The steps every plotted family's product kernel is instantiated with (draw_plot.h, CB_PLOT_STEPS), as (template, its
# argument): the reference's step and its Burning Ship variant, degrees 3 .. 8, formula codes 1 .. 5.
PLOT_STEPS = ([("ReferenceOrbit", "0"), ("ReferenceOrbit", "1")] + [("PowerOrbit", str(d)) for d in range(3, 9)]
              + [("FormulaOrbit", str(f)) for f in range(1, 6)])


def plot_instance_of(name, kernel, flags, args):
    """(step, flag, ...) of a mangled kernel<Step, bool x flags>(args): Step is ReferenceOrbit<bool> (ILb.E), PowerOrbit<int>
    or FormulaOrbit<int> (ILi.E); a flag is Lb0E or Lb1E; args is the argument type with its length, as mangled."""
    m = re.search(kernel + r"INS_\d+(ReferenceOrbit|PowerOrbit|FormulaOrbit)IL([bi])(\d+)EEE" + r"Lb(\d)E" * flags + "EEvNS_"
                  + args + "E$", name)
    assert m, name
    assert m.group(2) == ("b" if m.group(1) == "ReferenceOrbit" else "i"), name
    return ((m.group(1), m.group(3)),) + m.groups()[3:]
