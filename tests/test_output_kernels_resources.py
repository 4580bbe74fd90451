"""What the compiler makes of the output stage's kernels -- tonemap.hip, exposure.hip, equalize.hip (4.26),
density.hip (4.25), color.hip (4.5a) --, checked where it is built, the way tests/test_kernel_resources.py checks the draw
kernel.  One table, one row per file: exactly the kernels named, each with its LDS and its occupancy; no scratch, no
spilled register and no AGPR in any; the instructions a file must and must not hold; and the figures of the record under
profiles/<file>_kernel_usage.txt.  A bar that rests on a constant reads it from the file that defines it: the sweep's
from counter_sweep.h, the window from equalize.hip, the tile from density.hip.

  tonemap   the maximum and the three lookup kernels: no LDS, no fp64 (the map is evaluated on the host);
  exposure  the digit pass keeps its block-private bins at 256 u32 (1024 bytes), pass 0 one u64 pair per wave (64 bytes);
            the counters are read 16 bytes at a time, four loads in flight per lane, in both; no fp64 (the rank is the host's);
  equalize  the bins kernel's LDS is its window of u32 bins plus one u64 per wave for the maximum, at the occupancy DESIGN
            states for that window -- four waves per SIMD, the four blocks per CU its grid is capped at; no fp64 (the table
            is the host's); block-private bins, and the key a count-leading-zeros;
  density   full occupancy, no fp64 (the thresholds are the host's), one 64-bit multiply-add per tap, an LDS figure that is
            the staged tile (10 KiB), the two weight tables and the reach word, and 8 bytes per lane: aligned on every plane
            of an odd canvas;
  color     the two radix-select passes keep their LDS histograms at 256 bins (a 65536-bin one would not fit a CU), and no
            fused or approximate fp64 operation (include/cudabrot_amd.h allows none on the device)."""

import os
import re

import pytest

from kernel_resources import HIPCC, compile_kernels, matches_record, no_spill_no_scratch
from output_planted import source

SWEEP = source("counter_sweep.h")[1]
WINDOW = source("equalize.hip")[1]["kWindow"]
TILE = source("density.hip")[1]
WAVES = SWEEP["kSweepThreads"] // 64
NO_FP64 = r"\bv_\w+_f64\b"

# file: ({kernel: (LDS bytes or (least, most), waves per SIMD)}, patterns that must not match, {text: least count})
TABLE = {
    "tonemap": ({"hist_max_kernel": (0, 8), "tone_thresholds_kernel": (0, 8), "tone_lut_kernelILb0E": (0, 8),
                 "tone_lut_kernelILb1E": (0, 8)}, [NO_FP64], {}),
    "exposure": ({"exposure_max_lit_kernel": (64, 8), "exposure_digit_kernel": (1024, 8)}, [NO_FP64],
                 {"global_load_dwordx4": 2 * SWEEP["kLoads"]}),
    "equalize": ({"equalize_bins_kernel": (4 * WINDOW + 8 * WAVES, 4), "equalize_map_kernel": (0, 8)}, [NO_FP64],
                 {"global_load_dwordx4": SWEEP["kLoads"], "ds_add_u32": 1, "v_ffbh_u32": 1}),
    # the four arrays -- a halo of CB_DENSITY_MAX_RADIUS on every side, B_r[i] and B_r[i] << (32 - 4r) for r = 0 .. 8 and
    # i = -8 .. 8, the reach word -- and what the compiler pads between them
    "density": ({"density_filter_kernel": ((11468, 11468 + 16), 8)}, [NO_FP64, "scratch_", "global_load_dwordx4"],
                {"v_mad_u64_u32": 1}),
    "color": ({"color_coarse_kernel": (1024, 8), "color_fine_kernel": (2048, 8), "color_compose_kernel": (0, 8)},
              ["v_fma_f64", "v_fract_f64", "v_rcp_f64", "v_div_scale_f64"], {}),
}


def test_the_figures_the_table_rests_on():
    assert SWEEP == {"kSweepThreads": 256, "kSweepBlocks": 1024, "kLoads": 4, "kVector": 2}
    assert WINDOW % 1024 == 0 and WINDOW == 8192  # DESIGN 4.26's choice
    assert (TILE["kTileW"], TILE["kTileH"], TILE["kDensityThreads"]) == (64, 16, 256)
    assert 4 * ((TILE["kTileW"] + 16) * (TILE["kTileH"] + 16) + 2 * 9 * 17 + 1) == 11468


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
@pytest.mark.parametrize("name", sorted(TABLE))
def test_output_kernels_use_what_the_table_says(name):
    bars, absent, present = TABLE[name]
    kernels, assembly = compile_kernels(name)
    found = {n: k for k in kernels for n in bars if n in k["name"]}
    assert sorted(found) == sorted(bars) and len(kernels) == len(bars), [k["name"] for k in kernels]
    for n, k in found.items():
        lds, waves = bars[n]
        least, most = lds if isinstance(lds, tuple) else (lds, lds)
        assert no_spill_no_scratch(k), k
        assert int(k["AGPRs"]) == 0, k
        assert least <= int(k["LDS Size [bytes/block]"]) <= most, k
        assert int(k["Occupancy [waves/SIMD]"]) == waves, k
    for pattern in absent:
        assert not re.search(pattern, assembly), pattern
    for text, least in present.items():
        assert assembly.count(text) >= least, text
    matches_record(kernels, name)  # the record kept beside the other kernels' names the same figures
