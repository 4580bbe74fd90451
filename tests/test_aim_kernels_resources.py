"""What the compiler makes of the aimed render's kernels (draw_aim.hip: the un-aimed renders' modes behind the cell source on
draw_rounds.h's scheduler -- one instance of draw_aim_kernel per step, per source of c and per kind --, the four probe
kernels and the lock-step kernel), checked where it is built: hipcc cross-compiles for gfx950 without a GPU and reports every
kernel's resources (tests/kernel_resources.py).  The file is compiled once.  DESIGN.md 4.23 claims
no spill, no scratch, no AGPRs and no LDS for all 57, the plotted families' bar -- at most 128 VGPRs and at least 4 waves per
SIMD --, and the figures of profiles/draw_aim_kernel_usage.txt.  Judged from the compiler's reported figures only."""

import os
import re

import pytest

from kernel_resources import (HIPCC, PLOT_STEPS, at_most, compile_kernels, matches_record, no_spill_no_scratch,
                              plot_instance_of, row)

BAR = at_most(128, 4)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_aim_kernels_fit_without_scratch_and_match_the_record():
    kernels, _ = compile_kernels("draw_aim")
    product = [k for k in kernels if "draw_aim_kernel" in k["name"]]
    probe = [k for k in kernels if "draw_aim_probe_kernel" in k["name"]]
    lockstep = [k for k in kernels if "draw_aim_simple_kernel" in k["name"]]
    # 52 aimed draws, 4 probes, the lock-step kernel, nothing else
    assert len(product) == 52 and len(probe) == 4 and len(lockstep) == 1 and len(kernels) == 57, [k["name"] for k in kernels]
    for k in kernels:
        print(row(k))
        assert no_spill_no_scratch(k), k
        assert int(k["AGPRs"]) == 0 and int(k["LDS Size [bytes/block]"]) == 0, k
        assert BAR(k), k
    # the exact instance sets: every step of CB_PLOT_STEPS x {sampled c, fixed c} x {escaping, bounded}; the probes by
    # source of c and kind alone
    instances = sorted(plot_instance_of(k["name"], "draw_aim_kernel", 2, "7AimArgs") for k in product)
    assert instances == sorted((s, j, b) for s in PLOT_STEPS for j in "01" for b in "01")
    probes = sorted(re.search(r"draw_aim_probe_kernelILb(\d)ELb(\d)EEEvNS_7AimArgsE$", k["name"]).groups() for k in probe)
    assert probes == sorted((j, b) for j in "01" for b in "01")
    matches_record(kernels, "draw_aim")  # the committed record says what the compiler says
