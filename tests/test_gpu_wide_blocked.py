"""draw_wide_kernel's BLOCKED pixel stream (draw_wide.hip, CBW_REPLAY_LOOP_BLOCKED; kernels.h, kStreamBlocked): a lane's
points of four consecutive replay steps leave in one 16-byte block, and the region sort skips the slots that hold none.

The bar of tests/test_gpu_wide.py -- every pixel and every counter, `increments` among them, against the oracle AND against
draw_wave_kernel (which writes single words) on the same launches -- at the places where the blocks can go wrong: one
and two workgroups, the power-of-two and the dividing pixel text, a crop on which most orbit points fall outside (empty
slots inside otherwise full blocks), orbits of 200 to 2000 steps, sample counts at which bursts end in the middle of a
group and a drain launch that runs bursts of a few lanes, two carried launches before the drain, and a workspace so
small that the waves' regions fill up and the burst turns to direct atomics in mid-launch.
"""

import numpy as np
import pytest

from device_launches import SQUARE, Launches, assert_same, omp_threads

pytestmark = pytest.mark.gpu

WIDE, WAVE = 2, 1
CROP = (-0.9, -0.55, 0.05, 0.3)  # a window on the seahorse valley: nearly every point of an orbit lies outside it
HALF = (-1.0, 0.25, -0.5, 0.5)   # ... and one that about half of them miss


def _launches(cb, w, h, box, max_iter, threads, samples, workspace_samples):
    dims = cb.FractalDimensions.make(w, h, *box)
    it = cb.IterationControl(max_iter, 20)
    ws = cb.scatter_workspace_bytes(dims, threads, workspace_samples)
    assert ws > 0
    seq = Launches(cb, dims, threads, workspace=ws, carry=True)
    kernels = {seq.launch(cb.draw_buddhabrot, n, iterations=it) for n in samples}
    hist, cnt = seq.read()[:2]
    return hist, cnt, kernels


CASES = {
    # w, h, box, max_iter, passes of the two carried launches (50 samples each; the drain follows), workspace (samples)
    "pow2_512": (256, 256, SQUARE, 500, (1, 2), None, 512),
    "pow2_1024": (256, 256, SQUARE, 2000, (3, 1), None, 1024),
    "dividing_512": (333, 77, (-1.7, 0.9, -0.3, 1.1), 1234, (2, 3), None, 512),
    "dividing_1024": (333, 77, (-1.7, 0.9, -0.3, 1.1), 200, (1, 1), None, 1024),
    "crop_pow2": (256, 256, CROP, 2000, (2, 2), None, 1024),
    "crop_dividing": (300, 200, HALF, 800, (1, 3), None, 512),
    "small_workspace": (256, 256, SQUARE, 2000, (12, 12), 200, 1024),
}


@pytest.mark.parametrize("name", CASES)
def test_blocked_stream_equals_oracle_and_wave_kernel(cb, oracle, monkeypatch, name):
    w, h, box, max_iter, passes, ws_samples, threads = CASES[name]
    samples = [50 * p for p in passes] + [0]
    ws_samples = ws_samples or max(samples)
    wide = _launches(cb, w, h, box, max_iter, threads, samples, ws_samples)
    assert wide[2] == {WIDE}, "a launch was not taken by draw_wide_kernel"
    monkeypatch.setenv("CUDABROT_AMD_NO_WIDE", "1")
    wave = _launches(cb, w, h, box, max_iter, threads, samples, ws_samples)
    assert wave[2] == {WAVE}
    assert_same(wide, wave, what=name + " (wide, wave)")
    ref = oracle.render(w, h, max_iter, 20, threads, sum(passes), box, omp_threads=omp_threads())
    assert_same(wide, ref, what=name + " (wide, oracle)")
    assert wide[1]["increments"] == int(ref[0].sum()) > 0
    if name == "small_workspace":  # the stream has room for a part of the increments: the rest went the direct way
        dims = cb.FractalDimensions.make(w, h, *box)
        layout = cb.debug_scatter_layout(dims, threads, 1 << 20, cb.scatter_workspace_bytes(dims, threads, ws_samples))
        assert layout.enabled and layout.cap * layout.n_waves < wide[1]["increments"]
    elif name.startswith("crop"):  # (a large share of the replayed points fall outside: slots without a point)
        assert 4 * wide[1]["increments"] < 3 * wide[1]["replay_steps"]
