"""What the compiler makes of the palette kernels (draw_palette.hip: the palette plot mode of draw_rounds.h's scheduler,
one instance per step and per source of c, and its lock-step twin), checked where it is built: hipcc cross-compiles for
gfx950 without a GPU and reports every kernel's resources (the method of tests/test_round_kernels_resources.py).
DESIGN.md section 4.14 claims no spill, no scratch, no AGPRs and no LDS for every instance, at most 128 VGPRs and at
least 4 waves per SIMD.  Judged from the compiler's reported figures only."""

import os
import re

import pytest

from test_round_kernels_resources import HIPCC, compile_kernels


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_palette_kernels_fit_without_scratch(tmp_path):
    kernels, _ = compile_kernels(tmp_path, "draw_palette")
    product = [k for k in kernels if "draw_palette_kernel" in k["name"]]
    lockstep = [k for k in kernels if "draw_palette_simple_kernel" in k["name"]]
    # sixteen product instances ({Mandelbrot step, Burning Ship, degrees 3 .. 8} x {sampled c, fixed c}); one lock-step
    # kernel; nothing else
    assert len(product) == 16 and len(lockstep) == 1 and len(kernels) == 17, [k["name"] for k in kernels]
    for fixed in ("0", "1"):  # the second template argument: Lb0E sampled, Lb1E fixed
        half = [k for k in product if k["name"].endswith("ELb%sEEEvNS_11PaletteArgsE" % fixed)]
        reference = [k for k in half if "ReferenceOrbit" in k["name"]]
        power = [k for k in half if "PowerOrbit" in k["name"]]
        assert len(half) == 8, [k["name"] for k in half]
        assert sorted(re.search(r"ReferenceOrbitILb(\d)E", k["name"]).group(1) for k in reference) == ["0", "1"]
        assert sorted(re.search(r"PowerOrbitILi(\d+)E", k["name"]).group(1) for k in power) == ["3", "4", "5", "6", "7", "8"]
    for k in kernels:
        print(k["name"], "VGPRs", k["VGPRs"], "SGPRs", k["TotalSGPRs"], "waves/SIMD", k["Occupancy [waves/SIMD]"])
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0 and int(k["ScratchSize [bytes/lane]"]) == 0, k
        assert int(k["AGPRs"]) == 0 and int(k["LDS Size [bytes/block]"]) == 0, k
        assert int(k["VGPRs"]) <= 128 and int(k["Occupancy [waves/SIMD]"]) >= 4, k
