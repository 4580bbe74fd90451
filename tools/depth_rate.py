"""Depth-render throughput through cb_renderer: samples per second and executed steps per sample on a
4096^2 canvas over [-2, 2]^2 with the identity plane, 262144 threads, -c 20, at -m 500 and -m 20000: the depth render
`cr:-2:0.5` at N = 1 and N = 64, product kernel (draw_depth_kernel, draw_depth.hip) and lock-step twin, and beside them the
projected render's product kernel (draw_plot_kernel) on the same shape.  Every measurement is a process of its own under
its own time limit (a child of this script); it makes one warm-up pass and then three timed repetitions, finish()
included, and prints one JSON line with the three rates and their median.  The first child that fails or runs out of time
ends the script: nothing more is started on the device after it.

    python tools/depth_rate.py [--slices 1,64] [--max-iters 500,20000] [--window -2:0.5] [-c 20] [--seconds 0.5] [--limit 120]

--window MIN:MAX is the depth window along c_re: -2:0.5 makes delta_d no power of two for any N (the kernel divides),
-2:2 makes it one for N = 1 and 64 (the kernel multiplies by the reciprocal, as it does for this canvas's pixels).
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


def measure(slices, max_iter, min_iter, side, seconds, lockstep, window):
    """slices 0: the projected render without a depth."""
    import cudabrot_amd as cb

    kernel = cb.CB_KERNEL_SIMPLE if lockstep else cb.CB_KERNEL_DEFAULT
    batch, max_batches = (1, 4) if lockstep else (4, 64)
    dims = cb.FractalDimensions.make(side, side)
    rates, steps = [], []
    with cb.Renderer(dims, cb.IterationControl(max_iter, min_iter), device=0, n_threads=cb.CB_DEFAULT_THREADS) as r:
        r.set_projection(cb.IDENTITY_PROJECTION)
        if slices:
            r.set_depth(("cr", window[0], window[1], slices))
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
        "what": ("depth" if slices else "projected") + (" lock-step" if lockstep else " product"),
        "kernel": drawn_by,
        "slices": slices,
        "window": list(window) if slices else None,
        "max_iter": max_iter,
        "msamples_per_s": rates,
        "median_msamples_per_s": statistics.median(rates),
        "executed_steps_per_sample": statistics.median(steps),
        "increments_per_sample": round(d["increments"] / d["samples"], 3),
        "status": after["status"],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", default="1,64")
    ap.add_argument("--max-iters", default="500,20000")
    ap.add_argument("--window", default="-2:0.5")
    ap.add_argument("-c", type=int, default=20)
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--limit", type=float, default=120.0, help="time limit of each child process, seconds")
    ap.add_argument("--one", nargs=3, metavar=("SLICES", "MAX_ITER", "LOCKSTEP"), help="(a child: one measurement)")
    a = ap.parse_args()
    window = tuple(float(v) for v in a.window.split(":"))
    if a.one:
        print(json.dumps(measure(int(a.one[0]), int(a.one[1]), a.c, a.side, a.seconds, a.one[2] == "1", window)), flush=True)
        return 0
    for max_iter in (int(v) for v in a.max_iters.split(",")):
        # the projected render's product kernel first, then each slice count, product and lock-step
        for slices, lockstep in [(0, 0)] + [(int(v), k) for v in a.slices.split(",") for k in (0, 1)]:
            cmd = [sys.executable, os.path.abspath(__file__), "-c", str(a.c), "--side", str(a.side), "--seconds",
                   str(a.seconds), "--window=" + a.window, "--one", str(slices), str(max_iter), str(lockstep)]
            try:
                rc = subprocess.run(cmd, timeout=a.limit).returncode
            except subprocess.TimeoutExpired:
                print("depth_rate: N=%d m=%d lockstep=%d ran past %g s: stopping" % (slices, max_iter, lockstep, a.limit),
                      flush=True)
                return 124
            if rc != 0:
                print("depth_rate: N=%d m=%d lockstep=%d ended with status %d: stopping" % (slices, max_iter, lockstep, rc),
                      flush=True)
                return rc if rc > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
