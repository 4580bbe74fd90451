"""What the compiler makes of equalize_local.hip's two kernels, checked where it is built, the way
tests/test_output_kernels_resources.py checks the other files of the output stage: exactly the two kernels, no scratch, no
spilled register and no AGPR in either, no fp64 instruction (the tables are the host's and the blend is integer); the bins
kernel's LDS is its window of u32 bins and nothing else, at the occupancy DESIGN states for it -- five blocks of four waves
on a CU, one more than the four its grid of kSweepBlocks asks for --; the counters are read 16 bytes at a time, kLoads loads
in flight; and the figures of the record under profiles/equalize_local_kernel_usage.txt.  The window is read from the file
that defines it."""

import os
import re

import pytest

from kernel_resources import HIPCC, compile_kernels, matches_record, no_spill_no_scratch
from output_planted import source

SWEEP = source("counter_sweep.h")[1]
WINDOW = source("equalize_local.hip")[1]["kLocalWindow"]
LDS_PER_CU = 160 * 1024  # gfx950


def test_the_figures_the_bars_rest_on():
    assert WINDOW == 8192 == source("equalize.hip")[1]["kWindow"]  # the window of 4.26
    assert source("equalize_local.hip")[1] == {"kLocalWindow": WINDOW}
    assert LDS_PER_CU // (4 * WINDOW) == 5 and SWEEP["kSweepThreads"] // 64 == 4


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_local_equalize_kernels_use_what_design_says():
    kernels, assembly = compile_kernels("equalize_local")
    found = {n: k for k in kernels for n in ("local_bins_kernel", "local_map_kernel") if n in k["name"]}
    assert sorted(found) == ["local_bins_kernel", "local_map_kernel"] and len(kernels) == 2, [k["name"] for k in kernels]
    for k in kernels:
        assert no_spill_no_scratch(k), k
        assert int(k["AGPRs"]) == 0, k
    bins, mapped = found["local_bins_kernel"], found["local_map_kernel"]
    assert int(bins["LDS Size [bytes/block]"]) == 4 * WINDOW
    assert int(bins["Occupancy [waves/SIMD]"]) == LDS_PER_CU // (4 * WINDOW)  # blocks per CU, four waves each on four SIMDs
    assert int(mapped["LDS Size [bytes/block]"]) == 0 and int(mapped["Occupancy [waves/SIMD]"]) == 8
    assert not re.search(r"\bv_\w+_f64\b", assembly)
    assert "scratch_" not in assembly
    assert assembly.count("global_load_dwordx4") >= SWEEP["kLoads"]
    assert assembly.count("ds_add_u32") >= 1 and assembly.count("v_ffbh_u32") >= 1  # block-private bins; the key a clz
    matches_record(kernels, "equalize_local")
