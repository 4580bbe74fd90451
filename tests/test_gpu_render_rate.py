"""tools/render_rate.py on the device, one run of the tool per family at the smallest shapes that still take every setup
branch: every case is measured by a child of the tool, prints its record and was drawn by the kernel that
include/cudabrot_amd.h documents for cb_debug_last_draw_kernel.  No rate is asserted: at this size it means nothing."""

import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

SMALL = ["--side", "64", "--threads", "1024", "--seconds", "0", "--reps", "1", "-c", "5"]
NORMAL = (1, 2)
# family -> (its options, the kernel of each case in order)
RUNS = {
    "anti": (["--max-iters", "200"], [4, 5]),
    "focus": (["-m", "200", "--level", "4", "--probe", "1"], [NORMAL, 6, 7]),
    "project": (["-m", "200"], [NORMAL, 8, 9]),
    "power": (["--degrees", "3", "--max-iters", "200"], [10, 11]),
    "julia": (["--cs=-0.8,0.156:none", "--max-iters", "200"], [12, 13, 8]),
    "palette": (["--planes", "0,3", "--max-iter", "200"], [8, 14]),
    "formula": (["--rows", "ship,tricorn,lockstep", "-m", "200"], [8, 16, 17]),
    "depth": (["--slices", "4", "--max-iters", "200"], [8, 18, 19]),
    "depth_palette": (["--slices", "4", "--max-iters", "200"], [18, 20, 21]),
    "frames": (["--frames", "2", "-m", "200", "--plain-seconds", "0"], [22, 8, 22, 12]),
    "phoenix": (["-m", "200"], [24, 24, 12, 24, 25]),
}
RECORD_KEYS = ("kernel", "status", "passes", "ms_per_pass", "msamples_per_s", "median_passes", "median_ms_per_pass",
               "median_msamples_per_s", "executed_steps_per_sample", "counted_steps_per_sample", "increments_per_sample",
               "mincrements_per_s", "never_escaped_fraction")


@pytest.mark.parametrize("family", list(RUNS))
def test_the_tool_measures_every_case_of_the_family(repo_root, family):
    options, kernels = RUNS[family]
    cmd = [sys.executable, os.path.join(repo_root, "tools", "render_rate.py"), family] + options + SMALL

    def run(extra):
        r = subprocess.run(cmd + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, cwd=repo_root)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        return [json.loads(line) for line in r.stdout.splitlines()]

    cases = run(["--list"])
    assert len(cases) == len(kernels) <= 7
    records = run([])
    assert len(records) == len(cases)
    for case, rec, kernel in zip(cases, records, kernels):
        assert {k: rec[k] for k in case} == case
        assert all(k in rec for k in RECORD_KEYS), rec
        assert ("cells" in rec) == bool(case["focus"])
        if case["focus"]:
            assert 0 < rec["cells"] <= rec["cells_total"] == 64 * 64 and rec["probe_seconds"] > 0
        assert rec["status"] == 0, rec
        assert len(rec["passes"]) == len(rec["ms_per_pass"]) == len(rec["msamples_per_s"]) == 1
        parts = case["sweep"] if case["separate"] else 1  # one batch per repetition and render
        assert rec["passes"] == [parts * case["batch"]] and rec["msamples_per_s"][0] > 0 and rec["ms_per_pass"][0] > 0
        assert rec["kernel"] in (kernel if isinstance(kernel, tuple) else (kernel,)), rec
