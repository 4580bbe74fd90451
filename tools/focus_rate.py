"""Focused-render throughput through cb_renderer: in-canvas increments per second on one crop, 4096^2
canvas, 262144 threads, of (a) the normal render of that crop, (b) the focused render with the product kernel and
(c) with the lock-step kernel.  One JSON line each; timed passes after one warm-up pass, finish() included.

    python tools/focus_rate.py [--box MINRE,MAXRE,MINIM,MAXIM] [-m 20000] [-c 20] [--seconds 0.5]
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import cudabrot_amd as cb  # noqa: E402


def measure(name, box, max_iter, min_iter, side, seconds, kernel, focus, max_batches=64):
    dims = cb.FractalDimensions.make(side, side, *box)
    with cb.Renderer(dims, cb.IterationControl(max_iter, min_iter), device=0, n_threads=cb.CB_DEFAULT_THREADS) as r:
        listed = total = 0
        probe_seconds = 0.0
        if focus:
            t0 = time.perf_counter()
            listed, total = r.set_focus(focus["level"], focus["probe"], focus["dilate"], kernel)
            probe_seconds = time.perf_counter() - t0
        r.prepare(kernel)
        r.render_passes(1, kernel)  # warm-up: code objects, first touch of the histogram
        r.finish()
        before = r.read_counters().as_dict()
        batch, passes = focus["batch"] if focus else 128, 0
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
        "max_iter": max_iter,
        "passes": passes,
        "seconds": round(dt, 4),
        "probe_seconds": round(probe_seconds, 4),
        "cells": listed,
        "cells_total": total,
        "msamples_per_s": round(d["samples"] / dt / 1e6, 2),
        "increments_per_sample": round(d["increments"] / d["samples"], 6),
        "mincrements_per_s": round(d["increments"] / dt / 1e6, 3),
        "executed_steps_per_sample": round((d["iterate_steps"] + d["replay_steps"] - d["skipped_steps"]) / d["samples"], 2),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--box", default="-0.2,0.0,-0.9,-0.7")
    ap.add_argument("-m", type=int, default=20000)
    ap.add_argument("-c", type=int, default=20)
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--level", type=int, default=8)
    ap.add_argument("--probe", type=int, default=64)
    ap.add_argument("--dilate", type=int, default=1)
    ap.add_argument("--lockstep-batch", type=int, default=1)
    a = ap.parse_args()
    box = tuple(float(x) for x in a.box.split(","))
    focus = {"level": a.level, "probe": a.probe, "dilate": a.dilate, "batch": 4}
    print(json.dumps(measure("normal", box, a.m, a.c, a.side, a.seconds, cb.CB_KERNEL_DEFAULT, None)), flush=True)
    print(json.dumps(measure("focus product", box, a.m, a.c, a.side, a.seconds, cb.CB_KERNEL_DEFAULT, focus)), flush=True)
    focus["batch"] = a.lockstep_batch
    print(json.dumps(measure("focus lock-step", box, a.m, a.c, a.side, a.seconds, cb.CB_KERNEL_SIMPLE, focus,
                             max_batches=4)), flush=True)


if __name__ == "__main__":
    main()
