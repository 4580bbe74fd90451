"""What the compiler makes of the colour stage's kernels (color.hip), checked where it is built, the
way tests/test_kernel_resources.py checks the draw kernel: no scratch and no spilled register in any of them, and the
two radix-select passes keep their LDS histograms at 256 bins (a 65536-bin one would not fit a CU)."""

import os

import pytest

from kernel_resources import HIPCC, compile_kernels, no_spill_no_scratch


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_color_kernels_use_no_scratch_and_small_lds():
    kernels, assembly = compile_kernels("color")
    lds = {"color_coarse_kernel": 1024, "color_fine_kernel": 2048, "color_compose_kernel": 0}
    found = {n: k for k in kernels for n in lds if n in k["name"]}
    assert sorted(found) == sorted(lds), [k["name"] for k in kernels]
    for name, k in found.items():
        assert no_spill_no_scratch(k), k
        assert int(k["LDS Size [bytes/block]"]) == lds[name], k
    # the definition allows no fused or approximate fp64 operation on the device (include/cudabrot_amd.h)
    for op in ("v_fma_f64", "v_fract_f64", "v_rcp_f64", "v_div_scale_f64"):
        assert op not in assembly, op
