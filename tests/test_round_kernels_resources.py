"""What the compiler makes of the kernels with one reference thread per lane (draw_anti.hip, draw_focus.hip: the modes
of draw_rounds.h's scheduler and their lock-step twins), checked where it is built: hipcc cross-compiles for gfx950
without a GPU and reports every kernel's resources.  DESIGN.md sections 4.9 and 4.10 claim no spill, no scratch, no
AGPRs and no LDS for every instance, and per file the registers and waves per SIMD below.  The plotted renders' kernels
(draw_plot.hip): tests/test_plot_kernels_resources.py."""

import os

import pytest

from kernel_resources import HIPCC, at_most, compile_kernels, no_spill_no_scratch

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
def test_round_kernels_fit_without_scratch(name):
    product_name, instances, product_bar, lockstep_name, lockstep_bar, total = FILES[name]
    kernels, assembly = compile_kernels(name)
    product = [k for k in kernels if product_name in k["name"]]
    lockstep = [k for k in kernels if lockstep_name in k["name"]]
    # the product instances, one lock-step kernel, nothing else
    assert len(product) == instances and len(lockstep) == 1 and len(kernels) == total, [k["name"] for k in kernels]
    for k in kernels:
        assert no_spill_no_scratch(k), k
        assert int(k["AGPRs"]) == 0 and int(k["LDS Size [bytes/block]"]) == 0, k
    for k in product:
        assert product_bar(k), k
    for k in lockstep:
        assert lockstep_bar(k), k
    assert "scratch_" not in assembly
