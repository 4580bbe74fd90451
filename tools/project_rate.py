"""Projected-render throughput through cb_renderer: samples per second, executed steps per sample and
increments per second on a 4096^2 canvas over [-2, 2]^2, 262144 threads, of (a) the normal render, (b) the projected
render with the product kernel and (c) with its lock-step twin.  One JSON line each; timed passes after one warm-up pass,
finish() included.  The default matrix is the identity, so that all three put the same increments on the same canvas.

    python tools/project_rate.py [-m 20000] [-c 20] [--seconds 0.5] [--project a,b,c,d:e,f,g,h]
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import cudabrot_amd as cb  # noqa: E402


def measure(name, max_iter, min_iter, side, seconds, kernel, projection, batch, max_batches):
    dims = cb.FractalDimensions.make(side, side)
    with cb.Renderer(dims, cb.IterationControl(max_iter, min_iter), device=0, n_threads=cb.CB_DEFAULT_THREADS) as r:
        if projection is not None:
            r.set_projection(projection)
        r.prepare(kernel)
        r.render_passes(1, kernel)  # warm-up: code objects, the interior map, first touch of the histogram
        r.finish()
        drawn_by = cb.lib.cb_debug_last_draw_kernel()
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
    d = {k: after[k] - before[k] for k in ("samples", "recorded", "iterate_steps", "replay_steps", "increments",
                                           "skipped_steps")}
    return {
        "what": name,
        "kernel": drawn_by,
        "max_iter": max_iter,
        "passes": passes,
        "seconds": round(dt, 4),
        "msamples_per_s": round(d["samples"] / dt / 1e6, 2),
        "increments_per_sample": round(d["increments"] / d["samples"], 6),
        "mincrements_per_s": round(d["increments"] / dt / 1e6, 3),
        "executed_steps_per_sample": round((d["iterate_steps"] + d["replay_steps"] - d["skipped_steps"]) / d["samples"], 2),
        "status": after["status"],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-m", type=int, default=20000)
    ap.add_argument("-c", type=int, default=20)
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--project", default="1,0,0,0:0,1,0,0")
    ap.add_argument("--skip-normal", action="store_true")
    ap.add_argument("--skip-lockstep", action="store_true")
    a = ap.parse_args()
    rows = a.project.split(":")
    p = [float.fromhex(x) if "0x" in x.lower() else float(x) for row in rows for x in row.split(",")]
    if len(rows) != 2 or len(p) != 8:
        ap.error("--project wants a,b,c,d:e,f,g,h")
    if not a.skip_normal:
        print(json.dumps(measure("normal", a.m, a.c, a.side, a.seconds, cb.CB_KERNEL_DEFAULT, None, 128, 64)), flush=True)
    print(json.dumps(measure("project product", a.m, a.c, a.side, a.seconds, cb.CB_KERNEL_DEFAULT, p, 4, 64)), flush=True)
    if not a.skip_lockstep:
        print(json.dumps(measure("project lock-step", a.m, a.c, a.side, a.seconds, cb.CB_KERNEL_SIMPLE, p, 1, 4)),
              flush=True)


if __name__ == "__main__":
    main()
