"""What the compiler makes of the Multibrot kernels (draw_power.hip: a mode of draw_rounds.h's scheduler, one instance per
degree, and its lock-step twin), checked where it is built: hipcc cross-compiles for gfx950 without a GPU and reports
every kernel's resources (the method of tests/test_round_kernels_resources.py).  DESIGN.md section 4.12 claims no spill,
no scratch, no AGPRs and no LDS for every instance, at most 128 VGPRs and at least 4 waves per SIMD."""

import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cudabrot_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_power_kernels_fit_without_scratch(tmp_path):
    flags = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950", "-S",
             "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run([HIPCC, *flags, "-o", str(tmp_path / "kernels.s"), os.path.join(CSRC, "draw_power.hip")],
                         capture_output=True, text=True, cwd=CSRC)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels, cur = [], None
    for line in out.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
        if not m:
            continue
        body = m.group(1).strip()
        if body.startswith("Function Name:"):
            cur = {"name": body.split(":", 1)[1].strip()}
            kernels.append(cur)
        elif cur is not None and ":" in body:
            k, v = body.split(":", 1)
            cur[k.strip()] = v.strip()
    product = [k for k in kernels if "draw_power_kernel" in k["name"]]
    lockstep = [k for k in kernels if "draw_power_simple_kernel" in k["name"]]
    # six product instances, one per degree; one lock-step kernel; nothing else
    assert len(product) == 6 and len(lockstep) == 1 and len(kernels) == 7, [k["name"] for k in kernels]
    assert sorted(re.search(r"ILi(\d+)E", k["name"]).group(1) for k in product) == ["3", "4", "5", "6", "7", "8"]
    for k in product + lockstep:
        print(k["name"], "VGPRs", k["VGPRs"], "SGPRs", k["TotalSGPRs"], "waves/SIMD", k["Occupancy [waves/SIMD]"])
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0 and int(k["ScratchSize [bytes/lane]"]) == 0, k
        assert int(k["AGPRs"]) == 0 and int(k["LDS Size [bytes/block]"]) == 0, k
        assert int(k["VGPRs"]) <= 128 and int(k["Occupancy [waves/SIMD]"]) >= 4, k
    with open(tmp_path / "kernels.s") as f:
        assert "scratch_" not in f.read()
