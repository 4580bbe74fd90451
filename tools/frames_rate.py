"""Frames-render cost through cb_renderer: time per pass of the frames render with F matrices against F
projected (or Julia) renders of the same matrices, one after another, on a 1024^2 canvas over [-2, 2]^2, 262144 threads,
seed 1337, -m 2000 -c 20.  The matrices are the sweep zi,cr:0:90:F of the identity plane; F = 1, 8, 64; the Mandelbrot
step on a sampled c and the Julia set of c = (-0.8, 0.156).  Every measurement is a process of its own under its own time
limit (a child of this script); it makes one warm-up pass and then whole batches of passes for at least --seconds,
finish() included, and prints one JSON line.  The first child that fails or runs out of time ends the script: nothing
more is started on the device after it.

    python tools/frames_rate.py [--frames 1,8,64] [--sources sampled,julia] [-m 2000] [-c 20] [--side 1024]
                                [--seconds 0.5] [--plain-seconds 0.5] [--limit 240]

--plain-seconds is the time each of the F separate renders is measured for (F = 64 makes 64 of them).
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


def timed(cb, dims, it, kernel, julia, seconds, matrix, frames=None):
    """One renderer with `matrix` (and `frames`): warm-up pass, then whole batches for at least `seconds` -> (ms per
    pass, passes, counters delta, cb_debug_last_draw_kernel, status)."""
    batch, max_batches = 4, 64
    with cb.Renderer(dims, it, device=0, n_threads=cb.CB_DEFAULT_THREADS) as r:
        if julia:
            r.set_julia(C_JULIA, matrix)
        else:
            r.set_projection(matrix)
        if frames is not None:
            r.set_frames(frames)
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
            if dt >= seconds or passes >= max_batches * batch:
                break
        after = r.read_counters().as_dict()
    d = {k: after[k] - before[k] for k in ("samples", "increments")}
    return 1e3 * dt / passes, passes, d, drawn_by, after["status"]


def measure(n_frames, julia, separate, a):
    import cudabrot_amd as cb

    kernel = cb.CB_KERNEL_DEFAULT
    dims = cb.FractalDimensions.make(a.side, a.side)
    it = cb.IterationControl(a.m, a.c)
    mats, _ = cb.frames_from_sweep(cb.IDENTITY_PROJECTION, ("zi", "cr"), 0.0, 90.0, n_frames)
    out = {"what": "%d separate renders" % n_frames if separate else "frames render", "frames": n_frames,
           "source": "julia" if julia else "sampled", "max_iter": a.m}
    if not separate:
        ms, passes, d, drawn_by, status = timed(cb, dims, it, kernel, julia, a.seconds, cb.IDENTITY_PROJECTION, mats)
        out.update(ms_per_pass=round(ms, 3), passes=passes, kernel=drawn_by, status=status,
                   increments_per_sample=round(d["increments"] / d["samples"], 3))
        return out
    total, each, status = 0.0, [], 0
    for p in mats:  # a renderer of its own per frame: what F runs with --rotate do
        ms, passes, d, drawn_by, st = timed(cb, dims, it, kernel, julia, a.plain_seconds, p)
        total += ms
        each.append(round(ms, 3))
        status |= st
    out.update(ms_per_pass=round(total, 3), each_ms=each if n_frames <= 8 else [min(each), max(each)], kernel=drawn_by,
               status=status)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="1,8,64")
    ap.add_argument("--sources", default="sampled,julia")
    ap.add_argument("-m", type=int, default=2000)
    ap.add_argument("-c", type=int, default=20)
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--plain-seconds", type=float, default=0.5)
    ap.add_argument("--limit", type=float, default=240.0, help="time limit of each child process, seconds")
    ap.add_argument("--one", nargs=3, metavar=("FRAMES", "JULIA", "SEPARATE"), help="(a child: one measurement)")
    a = ap.parse_args()
    if a.one:
        print(json.dumps(measure(int(a.one[0]), a.one[1] == "1", a.one[2] == "1", a)), flush=True)
        return 0
    for source in a.sources.split(","):
        for n in (int(v) for v in a.frames.split(",")):
            for separate in (0, 1):
                cmd = [sys.executable, os.path.abspath(__file__), "-m", str(a.m), "-c", str(a.c), "--side", str(a.side),
                       "--seconds", str(a.seconds), "--plain-seconds", str(a.plain_seconds), "--one", str(n),
                       "1" if source == "julia" else "0", str(separate)]
                try:
                    rc = subprocess.run(cmd, timeout=a.limit).returncode
                except subprocess.TimeoutExpired:
                    print("frames_rate: F=%d %s separate=%d ran past %g s: stopping" % (n, source, separate, a.limit),
                          flush=True)
                    return 124
                if rc != 0:
                    print("frames_rate: F=%d %s separate=%d ended with status %d: stopping" % (n, source, separate, rc),
                          flush=True)
                    return rc if rc > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
