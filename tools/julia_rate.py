"""Julia-render throughput through cb_renderer: samples per second and executed steps per sample on a
4096^2 canvas over [-2, 2]^2 with the identity matrix, 262144 threads, -c 20, -m 20000, of the product kernel
(draw_plot_kernel with a fixed c, draw_plot.hip) and its lock-step twin at c = (-1, 0) and c = (-0.8, 0.156), and of the projected
render's product kernel on the plane (zr, zi) (c = "none": the nearest workload that samples c).  Every measurement is a
process of its own under its own time limit (a child of this script); it makes one warm-up pass and then three timed
repetitions, finish() included, and prints one JSON line with the three rates and their median.  The first child that
fails or runs out of time ends the script: nothing more is started on the device after it.

    python tools/julia_rate.py [--cs=-1,0:-0.8,0.156:none] [--max-iters 20000] [-c 20] [--seconds 0.5] [--limit 120]
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


def measure(c, max_iter, min_iter, side, seconds, lockstep):
    import cudabrot_amd as cb

    kernel = cb.CB_KERNEL_SIMPLE if lockstep else cb.CB_KERNEL_DEFAULT
    batch, max_batches = (1, 4) if lockstep else (4, 64)
    dims = cb.FractalDimensions.make(side, side)
    rates, steps = [], []
    with cb.Renderer(dims, cb.IterationControl(max_iter, min_iter), device=0, n_threads=cb.CB_DEFAULT_THREADS) as r:
        if c is None:
            r.set_projection(cb.IDENTITY_PROJECTION)
        else:
            r.set_julia(c)
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
            d = {k: after[k] - before[k] for k in ("samples", "iterate_steps", "replay_steps", "skipped_steps")}
            rates.append(round(d["samples"] / dt / 1e6, 2))
            steps.append(round((d["iterate_steps"] + d["replay_steps"] - d["skipped_steps"]) / d["samples"], 2))
    return {
        "what": ("projected" if c is None else "julia") + (" lock-step" if lockstep else " product"),
        "kernel": drawn_by,
        "c": c,
        "max_iter": max_iter,
        "msamples_per_s": rates,
        "median_msamples_per_s": statistics.median(rates),
        "executed_steps_per_sample": statistics.median(steps),
        "status": after["status"],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cs", default="-1,0:-0.8,0.156:none", help="RE,IM of each c, colon-separated; none: the projected render")
    ap.add_argument("--max-iters", default="20000")
    ap.add_argument("-c", type=int, default=20)
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--limit", type=float, default=120.0, help="time limit of each child process, seconds")
    ap.add_argument("--one", nargs=2, metavar=("MAX_ITER", "LOCKSTEP"), help="(a child: one measurement, of --one-c)")
    ap.add_argument("--one-c", default="none", help="(a child: its c, as in --cs)")
    a = ap.parse_args()
    if a.one:
        c = None if a.one_c == "none" else tuple(float(v) for v in a.one_c.split(","))
        print(json.dumps(measure(c, int(a.one[0]), a.c, a.side, a.seconds, a.one[1] == "1")), flush=True)
        return 0
    for max_iter in (int(v) for v in a.max_iters.split(",")):
        for c in a.cs.split(":"):
            for lockstep in ((0,) if c == "none" else (0, 1)):
                cmd = [sys.executable, os.path.abspath(__file__), "-c", str(a.c), "--side", str(a.side), "--seconds",
                       str(a.seconds), "--one-c=" + c, "--one", str(max_iter), str(lockstep)]
                try:
                    rc = subprocess.run(cmd, timeout=a.limit).returncode
                except subprocess.TimeoutExpired:
                    print("julia_rate: c=%s m=%d lockstep=%d ran past %g s: stopping" % (c, max_iter, lockstep, a.limit),
                          flush=True)
                    return 124
                if rc != 0:
                    print("julia_rate: c=%s m=%d lockstep=%d ended with status %d: stopping" % (c, max_iter, lockstep, rc),
                          flush=True)
                    return rc if rc > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
