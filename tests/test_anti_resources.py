"""What the compiler makes of the anti-Buddhabrot's kernels (draw_anti.hip), checked where it is built: hipcc cross-compiles
for gfx950 without a GPU and reports every kernel's resources.  DESIGN.md section 4.9 claims no spill, no scratch and at
least 7 waves per SIMD for the product kernel (8 for the lock-step one)."""

import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cudabrot_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_anti_kernels_fit_without_scratch(tmp_path):
    flags = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950", "-S",
             "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run([HIPCC, *flags, "-o", str(tmp_path / "anti.s"), os.path.join(CSRC, "draw_anti.hip")],
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
    product = [k for k in kernels if "draw_anti_kernel" in k["name"]]
    lockstep = [k for k in kernels if "draw_anti_simple_kernel" in k["name"]]
    assert len(product) == 2 and len(lockstep) == 1, [k["name"] for k in kernels]  # <ship> x 2, runtime ship flag
    for k in product + lockstep:
        assert int(k["VGPRs Spill"]) == 0 and int(k["ScratchSize [bytes/lane]"]) == 0, k
        assert int(k["AGPRs"]) == 0 and int(k["LDS Size [bytes/block]"]) == 0, k
    for k in product:
        assert int(k["VGPRs"]) <= 72 and int(k["Occupancy [waves/SIMD]"]) >= 7, k
    for k in lockstep:
        assert int(k["VGPRs"]) <= 64 and int(k["Occupancy [waves/SIMD]"]) == 8, k
