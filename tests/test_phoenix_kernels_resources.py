"""What the compiler makes of the Phoenix render's kernels (draw_phoenix.hip: PhoenixMode on draw_rounds.h's scheduler,
one instance of draw_phoenix_kernel per source of c, and the lock-step kernel), checked where it is built: hipcc
cross-compiles for gfx950 without a GPU and reports every kernel's resources
(tests/kernel_resources.py).  DESIGN.md section 4.19 claims the bar every plotted family has -- no spill, no
scratch, no AGPRs, no LDS, at most 128 VGPRs and at least 4 waves per SIMD.  Judged from the compiler's reported figures
and the assembly's text only."""

import os
import re

import pytest

from kernel_resources import HIPCC, at_most, compile_kernels, no_spill_no_scratch, row


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_phoenix_kernels_fit_without_scratch_or_lds():
    kernels, assembly = compile_kernels("draw_phoenix")
    product = [k for k in kernels if "draw_phoenix_kernel" in k["name"]]
    lockstep = [k for k in kernels if "draw_phoenix_simple_kernel" in k["name"]]
    # two product instances, the lock-step kernel, nothing else
    assert len(product) == 2 and len(lockstep) == 1 and len(kernels) == 3, [k["name"] for k in kernels]
    # the exact instance set: draw_phoenix_kernel<false> (a sampled c) and <true> (a fixed one)
    flags = sorted(re.search(r"draw_phoenix_kernelILb(\d)EEEvNS_11PhoenixArgsE$", k["name"]).group(1) for k in product)
    assert flags == ["0", "1"]
    bar = at_most(128, 4)
    for k in kernels:
        print(row(k))
        assert no_spill_no_scratch(k), k
        assert int(k["AGPRs"]) == 0 and int(k["LDS Size [bytes/block]"]) == 0, k
        assert bar(k), k
    assert "scratch_" not in assembly
