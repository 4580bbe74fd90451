"""What the compiler makes of the kernels with one reference thread per lane (draw_anti.hip, draw_focus.hip: the modes
of draw_rounds.h's scheduler and their lock-step twins), checked where it is built: hipcc cross-compiles for gfx950
without a GPU and reports every kernel's resources.  DESIGN.md sections 4.9 and 4.10 claim no spill, no scratch, no
AGPRs and no LDS for every instance, and per file the registers and waves per SIMD below.  The plotted renders' kernels
(draw_plot.hip): tests/test_plot_kernels_resources.py."""

import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cudabrot_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def at_most(vgprs, waves):
    return lambda k: int(k["VGPRs"]) <= vgprs and int(k["Occupancy [waves/SIMD]"]) >= waves


def compile_kernels(tmp_path, name):
    """Every kernel of cudabrot_amd/csrc/<name>.hip as the compiler reports it: [{"name": mangled, remark: value}], and
    the assembly it wrote."""
    flags = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950", "-S",
             "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run([HIPCC, *flags, "-o", str(tmp_path / "kernels.s"), os.path.join(CSRC, name + ".hip")],
                         capture_output=True, text=True, cwd=CSRC)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels, cur = [], None
    for line in out.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
        if not m:
            continue
        body = m.group(1).strip()
        if body.startswith("Function Name:"):
            cur = {"name": body.split(":", 1)[1].strip()}
            kernels.append(cur)
        elif cur is not None and ":" in body:
            k, v = body.split(":", 1)
            cur[k.strip()] = v.strip()
    with open(tmp_path / "kernels.s") as f:
        return kernels, f.read()


# The steps every plotted family's product kernel is instantiated with (draw_plot.h, CB_PLOT_STEPS), as (template, its
# argument): the reference's step and its Burning Ship variant, degrees 3 .. 8, formula codes 1 .. 5.  For the resource
# tests of draw_plot.hip, draw_depth.hip and draw_depth_palette.hip.
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


# file -> (product kernel, its instances, its bar, lock-step kernel, its bar, kernels in the file)
FILES = {
    # <ship> x 2; the lock-step kernel takes the ship as a run-time flag
    "draw_anti": ("draw_anti_kernel", 2, at_most(72, 7), "draw_anti_simple_kernel",
                  lambda k: int(k["VGPRs"]) <= 64 and int(k["Occupancy [waves/SIMD]"]) == 8, 3),
    # (cells, histogram), (uniform, mask), (uniform, histogram), each for both steps
    "draw_focus": ("draw_focus_kernel", 6, at_most(128, 4), "draw_focus_simple_kernel", at_most(128, 4), 7),
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
@pytest.mark.parametrize("name", list(FILES))
def test_round_kernels_fit_without_scratch(tmp_path, name):
    product_name, instances, product_bar, lockstep_name, lockstep_bar, total = FILES[name]
    kernels, assembly = compile_kernels(tmp_path, name)
    product = [k for k in kernels if product_name in k["name"]]
    lockstep = [k for k in kernels if lockstep_name in k["name"]]
    # the product instances, one lock-step kernel, nothing else
    assert len(product) == instances and len(lockstep) == 1 and len(kernels) == total, [k["name"] for k in kernels]
    for k in kernels:
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0 and int(k["ScratchSize [bytes/lane]"]) == 0, k
        assert int(k["AGPRs"]) == 0 and int(k["LDS Size [bytes/block]"]) == 0, k
    for k in product:
        assert product_bar(k), k
    for k in lockstep:
        assert lockstep_bar(k), k
    assert "scratch_" not in assembly
