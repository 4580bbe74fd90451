"""A short run of tools/gpu_fuzz.py: random shapes, the product kernel (direct launches and the cb_renderer
object) against the lock-step validation kernel, identical histograms and counters demanded."""

import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", [11, 12])
def test_random_shapes_product_kernel_equals_lockstep_kernel(repo_root, seed):
    r = subprocess.run([sys.executable, os.path.join(repo_root, "tools", "gpu_fuzz.py"), "15", str(seed)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "histograms and counters identical" in r.stdout


@pytest.mark.parametrize("seed", [21, 22])
def test_random_anti_launches_product_kernel_equals_lockstep_kernel(repo_root, seed):
    """ANTI=1: draw_anti_kernel against draw_anti_simple_kernel on random canvases, M at the edges of the kernel's rounds
    and chunks, ragged thread counts, several launches.  Seeds 21 and 22: for both, trials of the first seconds have
    M >= 120 and compress cycles (skipped_steps > 0), which the second assertion demands."""
    import re

    r = subprocess.run([sys.executable, os.path.join(repo_root, "tools", "gpu_fuzz.py"), "15", str(seed)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300,
                       env=dict(os.environ, ANTI="1"))
    assert r.returncode == 0, r.stdout[-3000:]
    assert "histograms, counters and generator states identical" in r.stdout
    m = re.search(r"gpu_fuzz: (\d+) anti trials \((\d+) with skipped_steps > 0\)", r.stdout)
    assert m and int(m.group(1)) >= int(m.group(2)) >= 1, r.stdout[-3000:]
