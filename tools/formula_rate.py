"""Formula-render throughput through cb_renderer: samples per second and executed steps per sample on a
4096^2 canvas over [-2, 2]^2 with the identity matrix, 262144 threads, -m 2000, -c 20 (the method of
tools/julia_rate.py), of each of the five product instances of draw_plot_kernel over FormulaOrbit<F> with a sampled c and one plane
(draw_plot.hip), of the lock-step kernel (with the tricorn), and beside them, as the yardstick, of the Burning Ship
instance of draw_plot_kernel on the same shape: the closest existing kernel -- the same scheduler, no rejection, no
interior map -- whose assembly the formula render leaves alone.  Every row is a process of its own under its own time
limit (a child of this script); it makes one warm-up pass and then three timed repetitions, finish() included, and prints
one JSON line with the three rates and their median.  The first child that fails or runs out of time ends the script:
nothing more is started on the device after it.

    python tools/formula_rate.py [--rows ship,tricorn,...,lockstep] [-m 2000] [-c 20] [--seconds 0.5] [--limit 120]
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

FORMULAS = ("tricorn", "celtic", "buffalo", "perpendicular", "celtic-tricorn")
ROWS = ("ship",) + FORMULAS + ("lockstep",)


def measure(row, max_iter, min_iter, side, seconds):
    import cudabrot_amd as cb

    lockstep = row == "lockstep"
    if row == "ship":
        variant = cb.CB_KERNEL_DEFAULT | cb.CB_KERNEL_FLAG_BURNING_SHIP
    else:
        variant = (cb.CB_KERNEL_SIMPLE if lockstep else cb.CB_KERNEL_DEFAULT) | cb.CB_KERNEL_FORMULA("tricorn" if lockstep else row)
    batch, max_batches = (1, 4) if lockstep else (4, 64)
    dims = cb.FractalDimensions.make(side, side)
    rates, steps = [], []
    with cb.Renderer(dims, cb.IterationControl(max_iter, min_iter), device=0, n_threads=cb.CB_DEFAULT_THREADS) as r:
        r.set_projection(cb.IDENTITY_PROJECTION)
        r.prepare(variant)
        r.render_passes(1, variant)  # warm-up: code objects, first touch of the histogram
        r.finish()
        drawn_by = cb.lib.cb_debug_last_draw_kernel()
        for _ in range(3):
            before = r.read_counters().as_dict()
            passes = 0
            t0 = time.perf_counter()
            while True:  # whole batches until the time asked for has passed
                r.render_passes(batch, variant)
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
        "row": row,
        "kernel": drawn_by,
        "max_iter": max_iter,
        "msamples_per_s": rates,
        "median_msamples_per_s": statistics.median(rates),
        "spread_msamples_per_s": round(max(rates) - min(rates), 2),
        "executed_steps_per_sample": statistics.median(steps),
        "status": after["status"],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default=",".join(ROWS), help="of " + ", ".join(ROWS))
    ap.add_argument("-m", type=int, default=2000)
    ap.add_argument("-c", type=int, default=20)
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--limit", type=float, default=120.0, help="time limit of each child process, seconds")
    ap.add_argument("--one", metavar="ROW", help="(a child: one measurement)")
    a = ap.parse_args()
    if a.one:
        print(json.dumps(measure(a.one, a.m, a.c, a.side, a.seconds)), flush=True)
        return 0
    for row in a.rows.split(","):
        if row not in ROWS:
            print("formula_rate: no such row: %s" % row, flush=True)
            return 2
        cmd = [sys.executable, os.path.abspath(__file__), "-m", str(a.m), "-c", str(a.c), "--side", str(a.side),
               "--seconds", str(a.seconds), "--one", row]
        try:
            rc = subprocess.run(cmd, timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            print("formula_rate: %s ran past %g s: stopping" % (row, a.limit), flush=True)
            return 124
        if rc != 0:
            print("formula_rate: %s ended with status %d: stopping" % (row, rc), flush=True)
            return rc if rc > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
