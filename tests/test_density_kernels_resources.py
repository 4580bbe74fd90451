"""What the compiler makes of the density filter's kernel (density.hip), checked where it is built, the way
tests/test_exposure_kernels_resources.py checks the white clip: no scratch, no spilled register and no AGPR, full
occupancy, no fp64 instruction (the thresholds are made on the host), one 64-bit multiply-add per tap, and an LDS figure
that is the staged tile (10 KiB), the two weight tables and the reach word.  The figures are recorded in
profiles/density_kernel_usage.txt."""

import os
import re

import pytest

from kernel_resources import HIPCC, ROOT, compile_kernels, matches_record, no_spill_no_scratch


def constants():
    with open(os.path.join(ROOT, "cudabrot_amd", "csrc", "density.hip")) as f:
        text = f.read()
    said = {k: int(v) for k, v in re.findall(r"constexpr uint32_t (kTileW|kTileH|kDensityThreads) = (\d+);", text)}
    assert sorted(said) == ["kDensityThreads", "kTileH", "kTileW"]
    return said


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_density_kernel_uses_no_scratch_no_fp64_and_the_lds_it_says():
    kernels, assembly = compile_kernels("density")
    assert len(kernels) == 1 and "density_filter_kernel" in kernels[0]["name"], [k["name"] for k in kernels]
    k = kernels[0]
    c = constants()
    halo = (c["kTileW"] + 16) * (c["kTileH"] + 16)   # a halo of CB_DENSITY_MAX_RADIUS on every side
    tables = 2 * 9 * 17                              # B_r[i] and B_r[i] << (32 - 4r), r = 0 .. 8, i = -8 .. 8
    assert no_spill_no_scratch(k), k
    assert int(k["AGPRs"]) == 0, k
    lds = int(k["LDS Size [bytes/block]"])  # the four arrays, and what the compiler pads between them
    assert 4 * (halo + tables + 1) == 11468 <= lds <= 11468 + 16, k
    assert int(k["Occupancy [waves/SIMD]"]) == 8, k
    assert not re.search(r"\bv_\w+_f64\b", assembly)
    assert "scratch_" not in assembly
    assert "v_mad_u64_u32" in assembly
    assert "global_load_dwordx4" not in assembly  # 8 bytes per lane: aligned on every plane of an odd canvas
    matches_record(kernels, "density")
