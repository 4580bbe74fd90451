"""What the compiler makes of the bounded render's kernels (draw_bounded.hip: BoundedMode on draw_rounds.h's scheduler, one
instance of draw_bounded_kernel per step and per source of c, and the lock-step kernel), checked where it is built: hipcc
cross-compiles for gfx950 without a GPU and reports every kernel's resources (tests/kernel_resources.py).
The file is compiled once.  DESIGN.md 4.21 claims no spill, no scratch, no AGPRs and no LDS for all 27, the plotted families' bar -- at most 128 VGPRs and at least 4 waves per SIMD --, and the figures of
profiles/draw_bounded_kernel_usage.txt.  Judged from the compiler's reported figures and the assembly's text only."""

import os

import pytest

from kernel_resources import (HIPCC, PLOT_STEPS, at_most, compile_kernels, matches_record, no_spill_no_scratch,
                              plot_instance_of, row)

BAR = at_most(128, 4)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_bounded_kernels_fit_without_scratch_and_match_the_record():
    kernels, assembly = compile_kernels("draw_bounded")
    product = [k for k in kernels if "draw_bounded_kernel" in k["name"]]
    lockstep = [k for k in kernels if "draw_bounded_simple_kernel" in k["name"]]
    # 26 product instances, the lock-step kernel, nothing else
    assert len(product) == 26 and len(lockstep) == 1 and len(kernels) == 27, [k["name"] for k in kernels]
    for k in kernels:
        print(row(k))
        assert no_spill_no_scratch(k), k
        assert int(k["AGPRs"]) == 0 and int(k["LDS Size [bytes/block]"]) == 0, k
        assert BAR(k), k
    # the exact instance set: every step of CB_PLOT_STEPS x {sampled c, fixed c}
    instances = sorted(plot_instance_of(k["name"], "draw_bounded_kernel", 1, "8PlotArgs") for k in product)
    assert instances == sorted((s, j) for s in PLOT_STEPS for j in "01")
    assert "scratch_" not in assembly
    matches_record(kernels, "draw_bounded")  # the committed record says what the compiler says
