"""What the compiler makes of the formula kernels (draw_formula.hip: the plot modes of draw_rounds.h's scheduler over the
five formula steps, one instance per code, per source of c and per sink, and their lock-step twin), checked where it is
built: hipcc cross-compiles for gfx950 without a GPU and reports every kernel's resources (the method of
tests/test_round_kernels_resources.py).  DESIGN.md section 4.15 claims no spill, no scratch, no AGPRs and no LDS for
every instance, at most 128 VGPRs and at least 4 waves per SIMD: the bar of tests/test_palette_kernels_resources.py for
plot kernels.  Judged from the compiler's reported figures only."""

import os
import re

import pytest

from test_round_kernels_resources import HIPCC, compile_kernels


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_formula_kernels_fit_without_scratch(tmp_path):
    kernels, assembly = compile_kernels(tmp_path, "draw_formula")
    product = [k for k in kernels if "draw_formula_kernel" in k["name"]]
    lockstep = [k for k in kernels if "draw_formula_simple_kernel" in k["name"]]
    # twenty product instances ({five codes} x {sampled c, fixed c} x {one plane, the palette's three}); one lock-step
    # kernel; nothing else
    assert len(product) == 20 and len(lockstep) == 1 and len(kernels) == 21, [k["name"] for k in kernels]
    instances = sorted(re.search(r"draw_formula_kernelILi(\d)ELb(\d)ELb(\d)EEE", k["name"]).groups() for k in product)
    assert instances == sorted((str(f), j, p) for f in range(1, 6) for j in "01" for p in "01")
    for k in kernels:
        print(k["name"], "VGPRs", k["VGPRs"], "SGPRs", k["TotalSGPRs"], "waves/SIMD", k["Occupancy [waves/SIMD]"])
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0 and int(k["ScratchSize [bytes/lane]"]) == 0, k
        assert int(k["AGPRs"]) == 0 and int(k["LDS Size [bytes/block]"]) == 0, k
        assert int(k["VGPRs"]) <= 128 and int(k["Occupancy [waves/SIMD]"]) >= 4, k
    assert "scratch_" not in assembly
