"""What the compiler makes of the white clip's kernels (exposure.hip), checked where it is built, the way
tests/test_color_resources.py checks the colour stage: no scratch, no spilled register and no AGPR in either kernel, the
digit pass keeps its block-private bins at 256 u32 (1024 bytes), pass 0 keeps one u64 pair per wave (64 bytes), the
counters are read 16 bytes at a time, and no fp64 reaches the device (the rank is made on the host).  The figures are
recorded in profiles/exposure_kernel_usage.txt."""

import os
import re

import pytest

from kernel_resources import HIPCC, compile_kernels, matches_record, no_spill_no_scratch

LDS = {"exposure_max_lit_kernel": 64, "exposure_digit_kernel": 1024}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_exposure_kernels_use_no_scratch_small_lds_and_no_fp64():
    kernels, assembly = compile_kernels("exposure")
    found = {n: k for k in kernels for n in LDS if n in k["name"]}
    assert sorted(found) == sorted(LDS) and len(kernels) == len(LDS), [k["name"] for k in kernels]
    for name, k in found.items():
        assert no_spill_no_scratch(k), k
        assert int(k["AGPRs"]) == 0, k
        assert int(k["LDS Size [bytes/block]"]) == LDS[name], k
        assert int(k["Occupancy [waves/SIMD]"]) == 8, k
    assert not re.search(r"\bv_\w+_f64\b", assembly)
    assert assembly.count("global_load_dwordx4") >= 8  # four 16-byte loads in flight per lane, in both kernels
    matches_record(kernels, "exposure")  # the record kept beside the other kernels' names the same figures
