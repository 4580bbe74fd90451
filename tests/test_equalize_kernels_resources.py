"""What the compiler makes of the equalised image's kernels (equalize.hip), checked where it is built, the
way tests/test_exposure_kernels_resources.py checks the white clip's: exactly the two kernels, no scratch, no spilled
register and no AGPR in either, no fp64 on the device (the table is made on the host), the bins kernel's LDS equal to its
window of u32 bins plus one u64 per wave for the maximum -- at the occupancy DESIGN states for that window, four waves per
SIMD, which is the four blocks per CU its grid is capped at --, the counters read 16 bytes at a time.  The figures are
recorded in profiles/equalize_kernel_usage.txt."""

import os
import re

import pytest

from kernel_resources import HIPCC, ROOT, compile_kernels, matches_record, no_spill_no_scratch


def constants():
    with open(os.path.join(ROOT, "cudabrot_amd", "csrc", "equalize.hip")) as f:
        return {k: int(v) for k, v in re.findall(r"constexpr uint32_t (k\w+) = (\d+);", f.read())}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_equalize_kernels_use_no_scratch_the_window_s_lds_and_no_fp64():
    k = constants()
    window, waves = k["kWindow"], k["kEqualizeThreads"] // 64
    assert window % 1024 == 0 and window == 8192  # DESIGN 4.26's choice
    lds = {"equalize_bins_kernel": 4 * window + 8 * waves, "equalize_map_kernel": 0}
    occupancy = {"equalize_bins_kernel": 4, "equalize_map_kernel": 8}
    kernels, assembly = compile_kernels("equalize")
    found = {n: kern for kern in kernels for n in lds if n in kern["name"]}
    assert sorted(found) == sorted(lds) and len(kernels) == len(lds), [kern["name"] for kern in kernels]
    for name, kern in found.items():
        assert no_spill_no_scratch(kern), kern
        assert int(kern["AGPRs"]) == 0, kern
        assert int(kern["LDS Size [bytes/block]"]) == lds[name], kern
        assert int(kern["Occupancy [waves/SIMD]"]) == occupancy[name], kern
    assert not re.search(r"\bv_\w+_f64\b", assembly)
    assert assembly.count("global_load_dwordx4") >= k["kLoads"]  # the 16-byte loads a lane has in flight
    assert "ds_add_u32" in assembly and "v_ffbh_u32" in assembly  # block-private bins; the key is a count-leading-zeros
    matches_record(kernels, "equalize")  # the record kept beside the other kernels' names the same figures
