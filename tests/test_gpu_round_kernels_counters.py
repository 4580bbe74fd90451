"""The kernels on the round scheduler (draw_rounds.h: draw_anti_kernel, draw_focus_kernel, draw_plot_kernel) against
a recording of themselves, `skipped_steps` included.

Every other comparison of these kernels leaves `skipped_steps` out, because product and lock-step kernels legitimately
differ there; it is the one counter that a slip in the shared scheduler (the Brent schedule, the chunk-boundary test, the
idle-to-round-end rule) moves while histograms stay right.  Here every product instance, for both steps, must reproduce
the complete cb_counters, the histogram (the probe: the mask) and the final generator states recorded in
tests/golden/round_kernel_counters.json.

The recording was made with this file on an MI355X from the library of commit dfdb289 ("Add --project/--plane/--rotate"),
the last one in which each of the three kernels carried its own copy of the scheduler:
    CUDABROT_RECORD_ROUND_COUNTERS=tests/golden/round_kernel_counters.json python -m pytest -m gpu <this file>
writes the file instead of comparing.  It is never to be re-recorded from the code under test.

128 x 128 canvas over [-2, 2]^2; 4000 threads (ragged: one partly filled workgroup); launches of 50 and 37 samples per
thread on the same generators, seed 1337; max_iter 2000 = 33 chunks of 60 + 20, so that orbits meet the Brent saves at
chunk counts 1, 2, 3, 4, 6, 8, 12, 16 and 24 and the limit off a chunk boundary; min_iter 20.
"""

import hashlib
import json
import os

import numpy as np
import pytest

import plot_reference as plot
from device_launches import Launches, counter_names

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "round_kernel_counters.json")
RECORD = os.environ.get("CUDABROT_RECORD_ROUND_COUNTERS", "")

W = H = 128
BOX = (-2.0, 2.0, -2.0, 2.0)
THREADS, LAUNCHES, MAX_ITER, MIN_ITER = 4000, (50, 37), 2000, 20
LEVEL = 4  # of the cell list and of the probe's mask
PROJECTION = plot.HOLOGRAM
INSTANCES = ("anti", "focus_cells_hist", "focus_uniform_mask", "focus_uniform_hist", "project")
CASES = [(instance, ship) for instance in INSTANCES for ship in (False, True)]


def planted_cells(level):
    """test_gpu_focus.py's planted "edges" list: cells on the axes, the corners, and one above the seahorse valley."""
    n = 4 << level
    valley = (17 * n // 32) * n + 5 * n // 16
    return np.array([n // 2, n * (n // 2), n * (n // 2) + n - 1, n * (n - 1) + n // 2, 0, n * n - 1, valley],
                    dtype=np.uint32)


def digest(array):
    return hashlib.sha256(np.ascontiguousarray(array).tobytes()).hexdigest()[:16]


def run(cb, instance, ship):
    """The two launches of one product instance -> {"kernel", "counters" (all of cb_counters, in its order), "out" and "states"
    (digests of the histogram -- the probe: the mask -- and of the generator states)}."""
    probe = instance == "focus_uniform_mask"
    seq = Launches(cb, cb.FractalDimensions.make(W, H, *BOX), THREADS, words=(4 << LEVEL) ** 2 // 32 if probe else None,
                   tables={"cells": planted_cells(LEVEL)})
    variant = cb.CB_KERNEL_DEFAULT | (cb.CB_KERNEL_FLAG_BURNING_SHIP if ship else 0)
    cells = seq.tables["cells"]
    entry, args = {
        "anti": (cb.draw_buddhabrot, {}),
        "focus_cells_hist": (cb.draw_buddhabrot_focus, dict(level=LEVEL, d_cells=cells.data_ptr(), n_cells=cells.numel())),
        "focus_uniform_hist": (cb.draw_buddhabrot_focus, {}),
        "focus_uniform_mask": (cb.focus_probe, dict(level=LEVEL)),
        "project": (cb.draw_buddhabrot_projected, dict(projection=PROJECTION)),
    }[instance]
    seq.launches(entry, LAUNCHES, variant | (cb.CB_KERNEL_FLAG_ANTI if instance == "anti" else 0),
                 iterations=cb.IterationControl(MAX_ITER, MIN_ITER), **args)
    out, cnt, kernel, states = seq.read()
    return {
        "kernel": int(kernel),
        "counters": list(cnt.values()),  # in cb_counters' order
        "out": digest(out),
        "states": digest(states),
    }


@pytest.mark.parametrize("instance,ship", CASES, ids=["%s-%s" % (i, "ship" if s else "mandelbrot") for i, s in CASES])
def test_round_kernels_reproduce_the_recorded_counters(cb, instance, ship):
    got = run(cb, instance, ship)
    names = counter_names(cb)
    c = dict(zip(names, got["counters"]))
    print(instance, "ship" if ship else "mandelbrot", json.dumps(got))
    # the case tests something: the product kernel, and (uniform Mandelbrot samples) orbits retired at chunk boundaries
    assert got["kernel"] == {"anti": 4, "project": 8}.get(instance, 6)
    assert c["status"] == 0 and c["samples"] == THREADS * sum(LAUNCHES)
    if not ship and instance != "focus_cells_hist":
        assert c["skipped_steps"] > 0 and c["never_escaped"] > 0
    key = "%s-%s" % (instance, "ship" if ship else "mandelbrot")
    projection = [float(x).hex() for x in np.asarray(PROJECTION, dtype=np.float64).reshape(-1)]
    if RECORD:
        recorded = {}
        if os.path.exists(RECORD):
            with open(RECORD) as f:
                recorded = json.load(f)
        recorded["projection"] = projection
        recorded[key] = got
        with open(RECORD, "w") as f:
            json.dump(recorded, f, sort_keys=True, separators=(",", ":"))
            f.write("\n")
        return
    with open(GOLDEN) as f:
        want = json.load(f)
    assert projection == want["projection"]  # the matrix the recording was made with, to the bit
    assert c == dict(zip(names, want[key]["counters"]))
    assert got == want[key]
