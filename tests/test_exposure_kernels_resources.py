"""What the compiler makes of the white clip's kernels (exposure.hip), checked where it is built, the way
tests/test_color_resources.py checks the colour stage: no scratch, no spilled register and no AGPR in either kernel, the
digit pass keeps its block-private bins at 256 u32 (1024 bytes), pass 0 keeps one u64 pair per wave (64 bytes), the
counters are read 16 bytes at a time, and no fp64 reaches the device (the rank is made on the host).  The figures are
recorded in profiles/exposure_kernel_usage.txt."""

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cudabrot_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
LDS = {"exposure_max_lit_kernel": 64, "exposure_digit_kernel": 1024}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_exposure_kernels_use_no_scratch_small_lds_and_no_fp64(tmp_path):
    # the Makefile's HIPFLAGS
    flags = ["-O3", "-std=c++17", "-fPIC", "-Wall", "-Wextra", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950",
             "-Wno-unused-result", "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"]
    asm = tmp_path / "exposure.s"
    out = subprocess.run([HIPCC, *flags, "-o", str(asm), os.path.join(CSRC, "exposure.hip")],
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
    found = {n: k for k in kernels for n in LDS if n in k["name"]}
    assert sorted(found) == sorted(LDS) and len(kernels) == len(LDS), [k["name"] for k in kernels]
    for name, k in found.items():
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, k
        assert int(k["ScratchSize [bytes/lane]"]) == 0, k
        assert int(k["AGPRs"]) == 0, k
        assert int(k["LDS Size [bytes/block]"]) == LDS[name], k
        assert int(k["Occupancy [waves/SIMD]"]) == 8, k
    text = asm.read_text()
    assert not re.search(r"\bv_\w+_f64\b", text)
    assert text.count("global_load_dwordx4") >= 8  # four 16-byte loads in flight per lane, in both kernels
    # the record kept beside the other kernels' names the same figures
    record = {}
    with open(os.path.join(ROOT, "profiles", "exposure_kernel_usage.txt")) as f:
        for line in f:
            if line.startswith("#") or not line.strip():
                continue
            m = re.match(r"(\S+)\s+VGPR\s+(\d+) AGPR\s+(\d+) SGPR\s+(\d+) spill s/v 0/0 scratch (\d+) LDS (\d+) occ (\d+)$",
                         line.rstrip())
            assert m, line
            record[m.group(1)] = tuple(int(v) for v in m.groups()[1:])
    assert sorted(record) == sorted(k["name"] for k in kernels)
    for k in kernels:
        now = (int(k["VGPRs"]), int(k["AGPRs"]), int(k["TotalSGPRs"]), int(k["ScratchSize [bytes/lane]"]),
               int(k["LDS Size [bytes/block]"]), int(k["Occupancy [waves/SIMD]"]))
        assert record[k["name"]] == now, (k["name"], record[k["name"]], now)
    shutil.rmtree(tmp_path, ignore_errors=True)
