"""Depth-palette throughput through cb_renderer, by the method of tools/depth_rate.py: samples per second
and executed steps per sample on a 4096^2 canvas over [-2, 2]^2 with the identity plane, depth row c_re, 262144 threads,
-c 20, at -m 500 and -m 20000, window `cr:-2:2` (delta_d a power of two) at N = 64 and N = 256: the depth-palette render
with a three-stop gradient whose weights are all non-zero (three atomics per plotted point), product kernel
(draw_depth_palette_kernel, draw_depth_palette.hip) and lock-step twin, and beside them the yardstick, the depth render's
product kernel (draw_depth_kernel) at the same window and N.  Every measurement is a process of its own under its own time
limit (a child of this script); it makes one warm-up pass and then three timed repetitions, finish() included, and prints
one JSON line with the three rates and their median.  The first child that fails or runs out of time ends the script:
nothing more is started on the device after it.

    python tools/depth_palette_rate.py [--slices 64,256] [--max-iters 500,20000] [--window -2:2] [-c 20] [--seconds 0.5]
                                       [--limit 120] [--kinds depth,palette,lockstep]
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

KINDS = ("depth", "palette", "lockstep")  # the yardstick, the product kernel, its lock-step twin


def measure(kind, slices, max_iter, min_iter, side, seconds, window):
    import cudabrot_amd as cb

    lockstep = kind == "lockstep"
    kernel = cb.CB_KERNEL_SIMPLE if lockstep else cb.CB_KERNEL_DEFAULT
    batch, max_batches = (1, 4) if lockstep else (4, 64)
    dims = cb.FractalDimensions.make(side, side)
    depth = ("cr", window[0], window[1], slices)
    rates, steps = [], []
    with cb.Renderer(dims, cb.IterationControl(max_iter, min_iter), device=0, n_threads=cb.CB_DEFAULT_THREADS) as r:
        r.set_projection(cb.IDENTITY_PROJECTION)
        if kind == "depth":
            r.set_depth(depth)
        else:  # dark blue to orange to white: no weight is zero anywhere
            last = max(slices - 1, 1)
            lut = cb.palette_from_stops([(0, 0x01, 0x02, 0x30), (last // 2 if last > 1 else 0, 0xFF, 0x80, 0x01),
                                         (last, 0xFF, 0xFF, 0xFF)][0 if last > 1 else 1:], slices)
            assert all((int(v) >> s) & 0xFF for v in lut for s in (0, 8, 16))
            r.set_depth_palette(depth, lut)
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
            d = {k: after[k] - before[k] for k in ("samples", "iterate_steps", "replay_steps", "skipped_steps", "increments")}
            rates.append(round(d["samples"] / dt / 1e6, 2))
            steps.append(round((d["iterate_steps"] + d["replay_steps"] - d["skipped_steps"]) / d["samples"], 2))
    return {
        "what": {"depth": "depth product", "palette": "depth-palette product", "lockstep": "depth-palette lock-step"}[kind],
        "kernel": drawn_by,
        "slices": slices,
        "window": list(window),
        "max_iter": max_iter,
        "msamples_per_s": rates,
        "median_msamples_per_s": statistics.median(rates),
        "executed_steps_per_sample": statistics.median(steps),
        "increments_per_sample": round(d["increments"] / d["samples"], 3),
        "status": after["status"],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", default="64,256")
    ap.add_argument("--max-iters", default="500,20000")
    ap.add_argument("--window", default="-2:2")
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("-c", type=int, default=20)
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--limit", type=float, default=120.0, help="time limit of each child process, seconds")
    ap.add_argument("--one", nargs=3, metavar=("KIND", "SLICES", "MAX_ITER"), help="(a child: one measurement)")
    a = ap.parse_args()
    window = tuple(float(v) for v in a.window.split(":"))
    kinds = a.kinds.split(",")
    if any(k not in KINDS for k in kinds):
        ap.error("--kinds takes " + ", ".join(KINDS))
    if a.one:
        print(json.dumps(measure(a.one[0], int(a.one[1]), int(a.one[2]), a.c, a.side, a.seconds, window)), flush=True)
        return 0
    for max_iter in (int(v) for v in a.max_iters.split(",")):
        for slices in (int(v) for v in a.slices.split(",")):
            for kind in kinds:
                cmd = [sys.executable, os.path.abspath(__file__), "-c", str(a.c), "--side", str(a.side), "--seconds",
                       str(a.seconds), "--window=" + a.window, "--one", kind, str(slices), str(max_iter)]
                try:
                    rc = subprocess.run(cmd, timeout=a.limit).returncode
                except subprocess.TimeoutExpired:
                    print("depth_palette_rate: %s N=%d m=%d ran past %g s: stopping" % (kind, slices, max_iter, a.limit),
                          flush=True)
                    return 124
                if rc != 0:
                    print("depth_palette_rate: %s N=%d m=%d ended with status %d: stopping" % (kind, slices, max_iter, rc),
                          flush=True)
                    return rc if rc > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
