"""What the compiler makes of the depth render's kernels (draw_depth.hip: DepthMode on draw_rounds.h's scheduler, one
instance of draw_depth_kernel per step and per source of c, and the lock-step kernel), checked where it is built: hipcc
cross-compiles for gfx950 without a GPU and reports every kernel's resources (the method of
tests/test_plot_kernels_resources.py).  DESIGN.md section 4.16 claims no spill, no scratch, no AGPRs and no LDS for
every kernel, at most 128 VGPRs and at least 4 waves per SIMD -- the bar every plotted family has.  Judged from the
compiler's reported figures and the assembly's text only."""

import os

import pytest

from kernel_resources import HIPCC, PLOT_STEPS, at_most, compile_kernels, no_spill_no_scratch, plot_instance_of, row

INSTANCES = [(s, j) for s in PLOT_STEPS for j in "01"]  # 13 steps x {sampled c, fixed c}


def instance_of(name):
    """(step, fixed c) of a mangled draw_depth_kernel<Step, kJulia>: Lb0E sampled c, Lb1E fixed c."""
    return plot_instance_of(name, "draw_depth_kernel", 1, "9DepthArgs")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_depth_kernels_fit_without_scratch():
    kernels, assembly = compile_kernels("draw_depth")
    product = [k for k in kernels if "draw_depth_kernel" in k["name"]]
    lockstep = [k for k in kernels if "draw_depth_simple_kernel" in k["name"]]
    # 26 product instances, the lock-step kernel, nothing else
    assert len(product) == 26 and len(lockstep) == 1 and len(kernels) == 27, [k["name"] for k in kernels]
    bar = at_most(128, 4)
    for k in kernels:
        print(row(k))
        assert no_spill_no_scratch(k), k
        assert int(k["AGPRs"]) == 0 and int(k["LDS Size [bytes/block]"]) == 0, k
        assert bar(k), k
    assert sorted(instance_of(k["name"]) for k in product) == sorted(INSTANCES)  # the exact instance set
    assert "scratch_" not in assembly
