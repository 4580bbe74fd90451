"""What the compiler makes of the plotted renders' kernels (draw_plot.hip: the plot modes of draw_rounds.h's scheduler,
one instance of draw_plot_kernel per step, per source of c and per sink, and the five lock-step kernels), checked where
it is built: hipcc cross-compiles for gfx950 without a GPU and reports every kernel's resources
(tests/kernel_resources.py).  The file is compiled once.  DESIGN.md sections 4.11 to 4.15 claim, family by
family -- the projected render, the Multibrot step, the Julia render, the palette render, the formula step -- no spill,
no scratch, no AGPRs and no LDS for every instance, at most 128 VGPRs and at least 4 waves per SIMD: each family's bar is
stated on its own below -- and the figures of profiles/draw_plot_kernel_usage.txt.  Judged from the compiler's reported figures and the assembly's text only."""

import os

import pytest

from kernel_resources import (HIPCC, PLOT_STEPS, at_most, compile_kernels, matches_record, no_spill_no_scratch,
                              plot_instance_of, row)

LOCKSTEP = ["draw_project_simple_kernel", "draw_power_simple_kernel", "draw_julia_simple_kernel",
            "draw_palette_simple_kernel", "draw_formula_simple_kernel"]

# family -> (which product instances (step, fixed c, table) belong to it, its lock-step kernel, the bar of both);
# step: "ReferenceOrbit" / "PowerOrbit" / "FormulaOrbit" and its argument
FAMILIES = {
    "projected": (lambda s, j, p: s[0] == "ReferenceOrbit" and (j, p) == ("0", "0"), "draw_project_simple_kernel", at_most(128, 4)),
    "Multibrot": (lambda s, j, p: s[0] == "PowerOrbit" and (j, p) == ("0", "0"), "draw_power_simple_kernel", at_most(128, 4)),
    "Julia": (lambda s, j, p: s[0] != "FormulaOrbit" and (j, p) == ("1", "0"), "draw_julia_simple_kernel", at_most(128, 4)),
    "palette": (lambda s, j, p: s[0] != "FormulaOrbit" and p == "1", "draw_palette_simple_kernel", at_most(128, 4)),
    "formula": (lambda s, j, p: s[0] == "FormulaOrbit", "draw_formula_simple_kernel", at_most(128, 4)),
}
STEPS = PLOT_STEPS[:8]  # without a formula
# the instances of each family, as the render's own file instantiated them
INSTANCES = {
    "projected": [(s, "0", "0") for s in STEPS[:2]],                          # <ship> x 2
    "Multibrot": [(s, "0", "0") for s in STEPS[2:]],                          # one per degree
    "Julia": [(s, "1", "0") for s in STEPS],                                  # Mandelbrot step, Burning Ship, degrees 3 .. 8
    "palette": [(s, j, "1") for s in STEPS for j in "01"],                    # those eight x {sampled c, fixed c}
    "formula": [(s, j, p) for s in PLOT_STEPS[8:] for j in "01" for p in "01"],  # five codes x 2 x 2
}


def instance_of(name):
    """(step, fixed c, table) of a mangled draw_plot_kernel<Step, kJulia, kPalette>: Lb0E sampled c / one plane, Lb1E fixed
    c / the table."""
    return plot_instance_of(name, "draw_plot_kernel", 2, "8PlotArgs")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_plot_kernels_fit_without_scratch():
    kernels, assembly = compile_kernels("draw_plot")
    product = [k for k in kernels if "draw_plot_kernel" in k["name"]]
    lockstep = [k for k in kernels if "_simple_kernel" in k["name"]]
    # 52 product instances, the five lock-step kernels, nothing else
    assert len(product) == 52 and len(lockstep) == 5 and len(kernels) == 57, [k["name"] for k in kernels]
    for name in LOCKSTEP:
        assert len([k for k in lockstep if name in k["name"]]) == 1, name
    for k in kernels:
        print(row(k))
        assert no_spill_no_scratch(k), k
        assert int(k["AGPRs"]) == 0 and int(k["LDS Size [bytes/block]"]) == 0, k
    by_instance = {instance_of(k["name"]): k for k in product}
    assert len(by_instance) == 52
    seen = []
    for family, (belongs, lockstep_name, bar) in FAMILIES.items():
        mine = sorted(i for i in by_instance if belongs(*i))
        assert mine == sorted(INSTANCES[family]), (family, mine)  # the exact instance set of the family
        seen += mine
        for i in mine:
            assert bar(by_instance[i]), (family, by_instance[i])
        for k in lockstep:
            if lockstep_name in k["name"]:
                assert bar(k), (family, k)
    assert sorted(seen) == sorted(by_instance)  # every instance belongs to exactly one family
    assert "scratch_" not in assembly
    matches_record(kernels, "draw_plot")  # the committed record says what the compiler says
