"""Anti-Buddhabrot throughput through cb_renderer: Msamples/s of the cycle-compressed product kernel and of
the lock-step kernel, 4096^2 canvas, 262144 threads, at max_iter 500 and 20000.  One JSON line per (kernel, max_iter).

    python tools/anti_rate.py [--passes-product N] [--passes-lockstep N]
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import cudabrot_amd as cb  # noqa: E402


def measure(kernel, max_iter, passes, side=4096):
    variant = kernel | cb.CB_KERNEL_FLAG_ANTI
    dims = cb.FractalDimensions.make(side, side)
    with cb.Renderer(dims, cb.IterationControl(max_iter, 20), device=0, n_threads=cb.CB_DEFAULT_THREADS) as r:
        r.prepare(variant)
        r.render_passes(1, variant)  # warm-up: code objects, first touch of the histogram
        r.finish()
        before = r.read_counters().as_dict()
        t0 = time.perf_counter()
        r.render_passes(passes, variant)
        r.finish()
        dt = time.perf_counter() - t0
        after = r.read_counters().as_dict()
    d = {k: after[k] - before[k] for k in ("samples", "never_escaped", "iterate_steps", "replay_steps", "increments",
                                           "skipped_steps")}
    executed = d["iterate_steps"] + d["replay_steps"] - d["skipped_steps"]
    return {
        "kernel": "product" if kernel == cb.CB_KERNEL_DEFAULT else "lockstep",
        "max_iter": max_iter,
        "passes": passes,
        "seconds": round(dt, 4),
        "ms_per_pass": round(1e3 * dt / passes, 3),
        "msamples_per_s": round(d["samples"] / dt / 1e6, 2),
        "increments_per_s_G": round(d["increments"] / dt / 1e9, 3),
        "executed_steps_per_sample": round(executed / d["samples"], 2),
        "never_escaped_fraction": round(d["never_escaped"] / d["samples"], 5),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes-product", type=int, default=8)
    ap.add_argument("--passes-lockstep", type=int, default=1)
    ap.add_argument("--max-iters", default="500,20000")
    a = ap.parse_args()
    for m in (int(x) for x in a.max_iters.split(",")):
        for kernel, passes in ((cb.CB_KERNEL_DEFAULT, a.passes_product), (cb.CB_KERNEL_SIMPLE, a.passes_lockstep)):
            print(json.dumps(measure(kernel, m, passes)), flush=True)


if __name__ == "__main__":
    main()
