"""What the compiler makes of the depth-palette render's kernels (draw_depth_palette.hip: DepthPaletteMode on
draw_rounds.h's scheduler, one instance of draw_depth_palette_kernel per step and per source of c, and the lock-step
kernel), checked where it is built: hipcc cross-compiles for gfx950 without a GPU and reports every kernel's resources
(the method of tests/test_depth_kernels_resources.py).  DESIGN.md section 4.17 claims no spill, no scratch and no AGPRs
for every kernel, at most 128 VGPRs and at least 4 waves per SIMD -- the bar every plotted family has -- and, by the
decision taken there, the table staged in LDS: exactly 1024 bytes per block for every product instance (256 entries of
four bytes, one per thread of the workgroup), none for the lock-step kernel, which reads the table where it lies.  Judged
from the compiler's reported figures and the assembly's text only."""

import os

import pytest

from kernel_resources import HIPCC, PLOT_STEPS, at_most, compile_kernels, no_spill_no_scratch, plot_instance_of, row

INSTANCES = [(s, j) for s in PLOT_STEPS for j in "01"]  # 13 steps x {sampled c, fixed c}: draw_depth.hip's instance set


def instance_of(name):
    """(step, fixed c) of a mangled draw_depth_palette_kernel<Step, kJulia> (tests/test_depth_kernels_resources.py)."""
    return plot_instance_of(name, "draw_depth_palette_kernel", 1, "16DepthPaletteArgs")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_depth_palette_kernels_fit_without_scratch():
    kernels, assembly = compile_kernels("draw_depth_palette")
    product = [k for k in kernels if "draw_depth_palette_kernel" in k["name"]]
    lockstep = [k for k in kernels if "draw_depth_palette_simple_kernel" in k["name"]]
    # 26 product instances, the lock-step kernel, nothing else
    assert len(product) == 26 and len(lockstep) == 1 and len(kernels) == 27, [k["name"] for k in kernels]
    bar = at_most(128, 4)
    for k in kernels:
        print(row(k))
        assert no_spill_no_scratch(k), k
        assert int(k["AGPRs"]) == 0, k
        assert bar(k), k
    for k in product:
        assert int(k["LDS Size [bytes/block]"]) == 1024, k  # the staged table, and nothing else
    assert int(lockstep[0]["LDS Size [bytes/block]"]) == 0, lockstep[0]
    assert sorted(instance_of(k["name"]) for k in product) == sorted(INSTANCES)  # the exact instance set
    assert "scratch_" not in assembly
