"""A short run of tools/gpu_fuzz.py's PHOENIX mode: 100 random Phoenix launch sequences -- p, source of c, matrix,
canvas, window, iteration control, thread count and launches -- the product kernel (draw_phoenix_kernel) against the
lock-step kernel, identical histograms, counters and generator states demanded.  In a child process under its own time
limit, as tests/test_gpu_frames_fuzz.py does it."""

import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_random_phoenix_launches_product_kernel_equals_lockstep_kernel(repo_root):
    r = subprocess.run([sys.executable, os.path.join(repo_root, "tools", "gpu_fuzz.py"), "240", "41"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300,
                       env=dict(os.environ, PHOENIX="1", TRIALS="100"))
    assert r.returncode == 0, r.stdout[-3000:]
    assert "histograms, counters and generator states identical" in r.stdout
    m = re.search(r"gpu_fuzz: (\d+) phoenix trials \((\d+) with skipped_steps > 0, (\d+) with increments > 0\)", r.stdout)
    assert m and int(m.group(1)) == 100, r.stdout[-3000:]
    assert int(m.group(2)) >= 1 and int(m.group(3)) >= 10, r.stdout[-3000:]
