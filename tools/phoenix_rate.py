"""Phoenix-render rates through cb_renderer: time per pass, samples per second and executed steps per
sample on a 4096^2 canvas over [-2, 2]^2, -c 20, 262144 threads, seed 1337, at -m 500 and -m 2000, of
  (a) phoenix         the Phoenix product kernel (24) at p = (-0.5, 0), a sampled c;
  (b) phoenix_p0      the same at p = (0, 0);
  (c) julia           the Julia product kernel (12) at c = (-0.8, 0.156), and
      phoenix_julia   the Phoenix product kernel at p = (0, 0) on the same c: the same orbits, 7 against 11 fp64
                      instructions a step;
  (d) lockstep        the Phoenix lock-step kernel (25) at p = (-0.5, 0), a sampled c.
Every measurement is a process of its own under its own time limit (a child of this script); it makes one warm-up pass and
then whole batches of passes for at least --seconds, finish() included, and prints one JSON line.  The first child that
fails or runs out of time ends the script: nothing more is started on the device after it.

    python tools/phoenix_rate.py [--renders phoenix,phoenix_p0,julia,phoenix_julia,lockstep] [-m 500,2000] [-c 20]
                                 [--side 4096] [--seconds 0.5] [--limit 240]
"""

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C_JULIA = (-0.8, 0.156)
# name -> (fixed c, p or None for the Julia render itself, lock-step)
RENDERS = {
    "phoenix": (None, (-0.5, 0.0), False),
    "phoenix_p0": (None, (0.0, 0.0), False),
    "julia": (C_JULIA, None, False),
    "phoenix_julia": (C_JULIA, (0.0, 0.0), False),
    "lockstep": (None, (-0.5, 0.0), True),
}


def measure(name, max_iter, a):
    import cudabrot_amd as cb

    c, p, lockstep = RENDERS[name]
    kernel = cb.CB_KERNEL_SIMPLE if lockstep else cb.CB_KERNEL_DEFAULT
    dims = cb.FractalDimensions.make(a.side, a.side)
    batch, max_batches = (1, 16) if lockstep else (4, 64)
    with cb.Renderer(dims, cb.IterationControl(max_iter, a.c), device=0, n_threads=cb.CB_DEFAULT_THREADS) as r:
        if c is None:
            r.set_projection(cb.IDENTITY_PROJECTION)
        else:
            r.set_julia(c)
        if p is not None:
            r.set_phoenix(p)
        r.prepare(kernel)
        r.render_passes(1, kernel)  # warm-up: code objects, first touch of the histogram
        r.finish()
        drawn_by = cb.lib.cb_debug_last_draw_kernel()
        before = r.read_counters().as_dict()
        passes = 0
        t0 = time.perf_counter()
        while True:
            r.render_passes(batch, kernel)
            r.finish()
            passes += batch
            dt = time.perf_counter() - t0
            if dt >= a.seconds or passes >= max_batches * batch:
                break
        after = r.read_counters().as_dict()
    d = {k: after[k] - before[k] for k in ("samples", "iterate_steps", "replay_steps", "skipped_steps", "increments")}
    executed = d["iterate_steps"] + d["replay_steps"] - d["skipped_steps"]
    return {"render": name, "max_iter": max_iter, "kernel": drawn_by, "status": after["status"], "passes": passes,
            "ms_per_pass": round(1e3 * dt / passes, 3), "msamples_per_s": round(d["samples"] / dt / 1e6, 1),
            "executed_steps_per_sample": round(executed / d["samples"], 2),
            "counted_steps_per_sample": round((d["iterate_steps"] + d["replay_steps"]) / d["samples"], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--renders", default=",".join(RENDERS))
    ap.add_argument("-m", default="500,2000")
    ap.add_argument("-c", type=int, default=20)
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--limit", type=float, default=240.0, help="time limit of each child process, seconds")
    ap.add_argument("--one", nargs=2, metavar=("RENDER", "MAX_ITER"), help="(a child: one measurement)")
    a = ap.parse_args()
    if a.one:
        print(json.dumps(measure(a.one[0], int(a.one[1]), a)), flush=True)
        return 0
    for max_iter in (int(v) for v in a.m.split(",")):
        for name in a.renders.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "-c", str(a.c), "--side", str(a.side), "--seconds",
                   str(a.seconds), "--one", name, str(max_iter)]
            try:
                rc = subprocess.run(cmd, timeout=a.limit).returncode
            except subprocess.TimeoutExpired:
                print("phoenix_rate: %s -m %d ran past %g s: stopping" % (name, max_iter, a.limit), flush=True)
                return 124
            if rc != 0:
                print("phoenix_rate: %s -m %d ended with status %d: stopping" % (name, max_iter, rc), flush=True)
                return rc if rc > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
