"""Palette-render throughput through cb_renderer: samples per second of the palette product kernel
(draw_plot_kernel with a table, draw_plot.hip) with one, two and three non-zero planes, beside cb_draw_buddhabrot_projected's
product kernel on the same shape -- which this render leaves alone: the yardstick.  4096^2 canvas over [-2, 2]^2, the
identity matrix, 262144 threads, -c 20, -m 2000 by default; tables R = 1 / R = G = 1 / R = G = B = 1 for every k, so
each in-canvas point costs one, two or three atomics and the work is otherwise the projected render's.  Every measurement
is a process of its own under its own time limit (a child of this script); it makes one warm-up pass and then three
timed repetitions, finish() included, and prints one JSON line with the three rates and their median.  The first child
that fails or runs out of time ends the script: nothing more is started on the device after it.

    python tools/palette_rate.py [--planes 0,1,2,3] [--max-iter 2000] [-c 20] [--julia RE,IM] [--seconds 0.5] [--limit 120]

planes 0 is the projected render (or, with --julia, the Julia render) without a palette.
"""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(planes, c, max_iter, min_iter, side, seconds):
    import numpy as np

    import cudabrot_amd as cb

    kernel = cb.CB_KERNEL_DEFAULT
    batch, max_batches = 4, 64
    dims = cb.FractalDimensions.make(side, side)
    rates, points = [], []
    with cb.Renderer(dims, cb.IterationControl(max_iter, min_iter), device=0, n_threads=cb.CB_DEFAULT_THREADS) as r:
        if c is None:
            r.set_projection(cb.IDENTITY_PROJECTION)
        else:
            r.set_julia(c)
        if planes:
            r.set_palette(np.full(max_iter, (0x010101 >> (8 * (3 - planes))), dtype=np.uint32))
        r.prepare(kernel)
        r.render_passes(1, kernel)  # warm-up: code objects, first touch of the histogram
        r.finish()
        drawn_by = cb.lib.cb_debug_last_draw_kernel()
        for _ in range(3):
            before = r.read_counters().as_dict()
            passes = 0
            t0 = time.perf_counter()
            while True:  # whole batches until the time asked for has passed
                r.render_passes(batch, kernel)
                r.finish()
                passes += batch
                dt = time.perf_counter() - t0
                if dt >= seconds or passes >= max_batches * batch:
                    break
            after = r.read_counters().as_dict()
            d = {k: after[k] - before[k] for k in ("samples", "increments")}
            rates.append(round(d["samples"] / dt / 1e6, 2))
            points.append(round(d["increments"] / dt / 1e9, 3))
    return {
        "what": ("julia" if c else "projected") + (" palette, %d plane(s)" % planes if planes else ", no palette"),
        "kernel": drawn_by,
        "max_iter": max_iter,
        "msamples_per_s": rates,
        "median_msamples_per_s": statistics.median(rates),
        "median_gatomics_per_s": statistics.median(points),  # every weight is 1: increments = atomics
        "status": after["status"],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", default="0,1,2,3", help="non-zero planes of each measurement; 0: no palette")
    ap.add_argument("--max-iter", type=int, default=2000)
    ap.add_argument("-c", type=int, default=20)
    ap.add_argument("--julia", default="none", help="RE,IM: a Julia render instead of a projected one")
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--limit", type=float, default=120.0, help="time limit of each child process, seconds")
    ap.add_argument("--one", type=int, help="(a child: one measurement, that many planes)")
    a = ap.parse_args()
    if a.one is not None:
        c = None if a.julia == "none" else tuple(float(v) for v in a.julia.split(","))
        print(json.dumps(measure(a.one, c, a.max_iter, a.c, a.side, a.seconds)), flush=True)
        return 0
    for planes in (int(v) for v in a.planes.split(",")):
        cmd = [sys.executable, os.path.abspath(__file__), "-c", str(a.c), "--side", str(a.side), "--seconds", str(a.seconds),
               "--max-iter", str(a.max_iter), "--julia=" + a.julia, "--one", str(planes)]
        try:
            rc = subprocess.run(cmd, timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            print("palette_rate: planes=%d ran past %g s: stopping" % (planes, a.limit), flush=True)
            return 124
        if rc != 0:
            print("palette_rate: planes=%d ended with status %d: stopping" % (planes, rc), flush=True)
            return rc if rc > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
