"""What the compiler makes of the colour stage's kernels (color.hip), checked where it is built, the
way tests/test_kernel_resources.py checks the draw kernel: no scratch and no spilled register in any of them, and the
two radix-select passes keep their LDS histograms at 256 bins (a 65536-bin one would not fit a CU)."""

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cudabrot_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_color_kernels_use_no_scratch_and_small_lds(tmp_path):
    flags = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950", "-S",
             "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"]
    asm = tmp_path / "color.s"
    out = subprocess.run([HIPCC, *flags, "-o", str(asm), os.path.join(CSRC, "color.hip")],
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
    lds = {"color_coarse_kernel": 1024, "color_fine_kernel": 2048, "color_compose_kernel": 0}
    found = {n: k for k in kernels for n in lds if n in k["name"]}
    assert sorted(found) == sorted(lds), [k["name"] for k in kernels]
    for name, k in found.items():
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, k
        assert int(k["ScratchSize [bytes/lane]"]) == 0, k
        assert int(k["LDS Size [bytes/block]"]) == lds[name], k
    # the definition allows no fused or approximate fp64 operation on the device (include/cudabrot_amd.h)
    text = asm.read_text()
    for op in ("v_fma_f64", "v_fract_f64", "v_rcp_f64", "v_div_scale_f64"):
        assert op not in text, op
    shutil.rmtree(tmp_path, ignore_errors=True)
