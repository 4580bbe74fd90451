"""What the compiler makes of the frames render's kernels (draw_frames.hip: FramesMode on draw_rounds.h's scheduler, one
instance of draw_frames_kernel per step and per source of c, and the lock-step kernel), checked where it is built: hipcc
cross-compiles for gfx950 without a GPU and reports every kernel's resources (the method of
tests/test_plot_kernels_resources.py).  DESIGN.md section 4.18 claims the bar every plotted family has -- no spill, no
scratch, no AGPRs, at most 128 VGPRs and at least 4 waves per SIMD -- and for LDS exactly the point queues of a block's
four waves: 128 records of (z_re, z_im, c_re, c_im) each where c is sampled, of (z_re, z_im) where it is fixed, and none
in the lock-step kernel.  Judged from the compiler's reported figures and the assembly's text only."""

import os

import pytest

from kernel_resources import HIPCC, PLOT_STEPS, at_most, compile_kernels, no_spill_no_scratch, plot_instance_of, row

INSTANCES = [(s, j) for s in PLOT_STEPS for j in "01"]  # 13 steps x {sampled c, fixed c}
WAVES, SLOTS, DOUBLE = 4, 128, 8
QUEUE_BYTES = {"0": WAVES * SLOTS * 4 * DOUBLE, "1": WAVES * SLOTS * 2 * DOUBLE}  # by fixed c: 16 KiB, 8 KiB


def instance_of(name):
    """(step, fixed c) of a mangled draw_frames_kernel<Step, kJulia>: Lb0E sampled c, Lb1E fixed c."""
    return plot_instance_of(name, "draw_frames_kernel", 1, "10FramesArgs")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_frames_kernels_fit_without_scratch_and_hold_exactly_their_queues():
    kernels, assembly = compile_kernels("draw_frames")
    product = [k for k in kernels if "draw_frames_kernel" in k["name"]]
    lockstep = [k for k in kernels if "draw_frames_simple_kernel" in k["name"]]
    # 26 product instances, the lock-step kernel, nothing else
    assert len(product) == 26 and len(lockstep) == 1 and len(kernels) == 27, [k["name"] for k in kernels]
    bar = at_most(128, 4)
    for k in kernels:
        print(row(k))
        assert no_spill_no_scratch(k), k
        assert int(k["AGPRs"]) == 0, k
        assert bar(k), k
    assert sorted(instance_of(k["name"]) for k in product) == sorted(INSTANCES)  # the exact instance set
    for k in product:
        assert int(k["LDS Size [bytes/block]"]) == QUEUE_BYTES[instance_of(k["name"])[1]], k
    assert int(lockstep[0]["LDS Size [bytes/block]"]) == 0
    assert "scratch_" not in assembly
    # the matrices are read with scalar loads: a whole matrix at a time, and no vector load of one in the frame loop
    assert "s_load_dwordx16" in assembly
