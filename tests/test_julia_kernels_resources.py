"""What the compiler makes of the Julia kernels (draw_julia.hip: the Julia plot mode of draw_rounds.h's scheduler, one
instance per step, and its lock-step twin), checked where it is built: hipcc cross-compiles for gfx950 without a GPU and
reports every kernel's resources (the method of tests/test_round_kernels_resources.py).  DESIGN.md section 4.13 claims
no spill, no scratch, no AGPRs and no LDS for every instance, at most 128 VGPRs and at least 4 waves per SIMD."""

import os
import re

import pytest

from test_round_kernels_resources import HIPCC, compile_kernels


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_julia_kernels_fit_without_scratch(tmp_path):
    kernels, assembly = compile_kernels(tmp_path, "draw_julia")
    product = [k for k in kernels if "draw_julia_kernel" in k["name"]]
    lockstep = [k for k in kernels if "draw_julia_simple_kernel" in k["name"]]
    # eight product instances (Mandelbrot step, Burning Ship, degrees 3 .. 8); one lock-step kernel; nothing else
    assert len(product) == 8 and len(lockstep) == 1 and len(kernels) == 9, [k["name"] for k in kernels]
    reference = [k for k in product if "ReferenceOrbit" in k["name"]]
    power = [k for k in product if "PowerOrbit" in k["name"]]
    assert sorted(re.search(r"ILb(\d)E", k["name"]).group(1) for k in reference) == ["0", "1"]
    assert sorted(re.search(r"ILi(\d+)E", k["name"]).group(1) for k in power) == ["3", "4", "5", "6", "7", "8"]
    for k in kernels:
        print(k["name"], "VGPRs", k["VGPRs"], "SGPRs", k["TotalSGPRs"], "waves/SIMD", k["Occupancy [waves/SIMD]"])
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0 and int(k["ScratchSize [bytes/lane]"]) == 0, k
        assert int(k["AGPRs"]) == 0 and int(k["LDS Size [bytes/block]"]) == 0, k
        assert int(k["VGPRs"]) <= 128 and int(k["Occupancy [waves/SIMD]"]) >= 4, k
    assert "scratch_" not in assembly
