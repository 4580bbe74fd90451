#!/usr/bin/env python3
"""gpu_fuzz.py -- randomized A/B of the product kernel against the lock-step validation kernel.

Both run on the GPU through the C ABI; `draw_simple_kernel` is one lane per reference thread with the
reference's arithmetic and direct atomics and is itself pinned against the oracle by the
test-suite.  Each trial draws a random shape -- canvas size and box (dyadic and non-dyadic pixel deltas,
off-centre and partly empty windows), iteration window, thread count (ragged), samples per launch, number
of launches (or the cb_renderer object with its pipelined launches, early reads and a resume into a new
renderer), with / without scatter workspace (suggested or deliberately short), with / without carry buffer
(then ended by a drain launch or the drain flag), Mandelbrot / Burning Ship, seed and first subsequence --
and demands identical histograms and counters.

    python tools/gpu_fuzz.py [SECONDS] [SEED]      exit 1 at the first mismatch (the trial is printed)
    HEAVY=1 python tools/gpu_fuzz.py ...           product-sized launches and canvases, deferred scatter
                                                   against direct atomics of the same kernel
    ANTI=1 python tools/gpu_fuzz.py ...            the anti-Buddhabrot (CB_KERNEL_FLAG_ANTI): draw_anti_kernel against
                                                   draw_anti_simple_kernel, generator states compared as well; M from
                                                   the edges of its rounds (12 steps) and chunks (60 steps)
    POWER=1 python tools/gpu_fuzz.py ...           the Multibrot render (CB_KERNEL_POWER): draw_plot_kernel (PowerOrbit<D>) against
                                                   draw_power_simple_kernel (draw_plot.hip) -- random degree,
                                                   shapes and matrices, generator states compared as well
    DEPTH=1 python tools/gpu_fuzz.py ...           the depth render (cb_draw_buddhabrot_depth): draw_depth_kernel against
                                                   draw_depth_simple_kernel (draw_depth.hip) -- random step, source of
                                                   c, canvas, window, matrix, depth row, depth window, N, thread count
                                                   and launches, generator states compared as well; TRIALS=N ends the
                                                   run after N trials where that comes before SECONDS
    DEPTHPALETTE=1 python tools/gpu_fuzz.py ...    the depth-palette render (cb_draw_buddhabrot_depth_palette):
                                                   draw_depth_palette_kernel against draw_depth_palette_simple_kernel
                                                   (draw_depth_palette.hip) -- DEPTH's trials with a random table of N
                                                   entries (random weights with zeros among them, one colour, one-hot,
                                                   noise in the bits that are not read), three planes; TRIALS as there
                                                   (and for ANTI and POWER: the five are rows of AB_MODES, one loop)
    FRAMES=1 python tools/gpu_fuzz.py ...          the frames render (cb_draw_buddhabrot_frames): draw_frames_kernel against
                                                   draw_frames_simple_kernel (draw_frames.hip) -- DEPTH's step, source
                                                   of c, canvas, window, thread count and launches with F <= 16 matrices
                                                   (a sweep, unit planes, random entries, copies of one); TRIALS as there
    PHOENIX=1 python tools/gpu_fuzz.py ...         the Phoenix render (cb_draw_buddhabrot_phoenix): draw_phoenix_kernel against
                                                   draw_phoenix_simple_kernel (draw_phoenix.hip) -- DEPTH's source of c,
                                                   canvas, window, matrix, iteration control, thread count and launches
                                                   with a random p (zero, real, the classic -0.5, the corners, anywhere
                                                   in [-2, 2]^2); TRIALS as there
    PERIODS=1 python tools/gpu_fuzz.py ...         the period-palette render (cb_draw_buddhabrot_periods): draw_periods_kernel
                                                   against draw_periods_simple_kernel (draw_periods.hip) -- DEPTH's step,
                                                   source of c, canvas, window, matrix, iteration control, thread count and
                                                   launches with a random table of 2 .. 1024 entries (zeros among them) and
                                                   a tolerance from 0 to 0x1p+10, three planes; TRIALS as there
"""
import os

os.environ["CUDABROT_AMD_DEBUG"] = "1"  # the knobs below are read only behind this gate (cb_debug_knob)
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import cudabrot_amd as cb
from gpu_launches import Launches  # beside this script: the launch scaffolding the GPU tests use too

COMPARED = ("samples", "rejected", "never_escaped", "too_fast", "recorded", "iterate_steps", "replay_steps",
            "increments", "status")


def canvas_and_box(rng, t):
    big = rng.random() < 0.15
    t["w"] = rng.choice([1, 2, 7, 64, 100, 128, 129, 255, 256, 333, 512, 640, 1000]) if not big else rng.choice([2048, 3000, 4096])
    t["h"] = rng.choice([1, 3, 8, 64, 100, 127, 128, 200, 256, 384, 512, 777, 1000]) if not big else rng.choice([1024, 2500, 4096])
    kind = rng.random()
    if kind < 0.4:
        t["box"] = (-2.0, 2.0, -2.0, 2.0)
    elif kind < 0.6:
        t["box"] = (-2.0, 1.0, -1.5, 1.5)
    elif kind < 0.8:   # random window, usually a non-dyadic delta
        cx, cy = rng.uniform(-1.5, 0.5), rng.uniform(-1.0, 1.0)
        rx, ry = rng.uniform(0.05, 2.0), rng.uniform(0.05, 2.0)
        t["box"] = (cx - rx, cx + rx, cy - ry, cy + ry)
    else:              # far from the set: almost nothing lands
        t["box"] = (1.0, 3.0, 1.0, 2.5)


def trial(rng):
    t = {}
    canvas_and_box(rng, t)
    t["max_iter"] = rng.choice([1, 2, 5, 19, 20, 21, 33, 64, 100, 257, 1000, 2000, 5000, 20000])
    t["min_iter"] = rng.choice([0, 1, 2, 19, 20, 21, 32, 40, 99, 1000, 30000])
    t["threads"] = rng.choice([1, 63, 64, 65, 200, 256, 1000, 1024, 4096, 5000, 16384])
    t["launch_samples"] = [rng.choice([1, 2, 7, 50, 64, 100, 150]) for _ in range(rng.randint(1, 4))]
    t["workspace"] = rng.choice(["suggested", "suggested", "short", "none"])
    t["carry"] = rng.choice(["none", "drain_launch", "drain_flag"])
    t["ship"] = rng.random() < 0.2
    t["seed"] = rng.choice([1337, 1337, 1, 0xdeadbeefcafe])
    t["first"] = rng.choice([0, 0, 1, 262144, 2097151])
    t["two_level"] = rng.random() < 0.2          # the large-canvas sort on any canvas (test knob)
    t["chunked"] = rng.random() < 0.7            # ... its level A by the draw kernel (chunked stream) or as a counting sort
    t["windows"] = None
    if rng.random() < 0.25:                      # fused multi-channel launch: plane j == a run with window j
        t["windows"] = [(rng.choice([30, 100, 400, 2500]), rng.choice([0, 5, 20, 50, 300])) for _ in range(rng.randint(1, 4))]
    if rng.random() < 0.35:
        # a launch draw_wide_kernel takes (draw_wide.hip): whole workgroups of 512 subsequences, min_iter at the start
        # of the LONG stage, one level or a chunked stream, one channel, a carry buffer, a workspace (suggested or short: a full stream
        # region makes the bursts add directly); tails of every length through max_iter
        t["threads"] = rng.choice([512, 1024, 2048, 4096, 16384])
        t["min_iter"] = 20
        t["max_iter"] = rng.choice([21, 33, 64, 79, 80, 81, 100, 140, 257, 1000, 2000, 5000, 20000])
        t["launch_samples"] = [rng.choice([30, 50, 64, 100, 150, 400]) for _ in range(rng.randint(1, 4))]
        t["workspace"] = rng.choice(["suggested", "suggested", "short"])
        t["carry"] = rng.choice(["drain_launch", "drain_flag"])
        t["two_level"] = rng.random() < 0.3      # (chunked stream: the wide kernel's chunked burst; a counting sort: draw_wave_kernel's)
        t["windows"] = None
    if t["max_iter"] >= 5000:   # keep the lock-step kernel's run time in hand
        t["threads"] = min(t["threads"], 4096)
    return t


def read(seq, on_device=False):
    """-> (histogram, flat; counters; generator states) of a finished launch sequence."""
    hist, cnt, _, states = seq.read(on_device)
    return hist.reshape(-1), cnt, states


def render(t, variant, window=None, fused=False, on_device=False):
    """window: (max, min) instead of the trial's; fused: all of t["windows"] in one launch (planes)."""
    dims = cb.FractalDimensions.make(t["w"], t["h"], *t["box"])
    planes = len(t["windows"]) if fused else 1
    n = t["threads"]
    flags = cb.CB_KERNEL_FLAG_BURNING_SHIP if t["ship"] else 0
    simple = variant == cb.CB_KERNEL_SIMPLE
    if t["two_level"] and not simple:
        os.environ["CUDABROT_AMD_TWO_LEVEL"] = "1"
    else:
        os.environ.pop("CUDABROT_AMD_TWO_LEVEL", None)
    os.environ["CUDABROT_AMD_CHUNKED"] = "1" if t.get("chunked", True) else "0"
    ws_bytes = 0
    if not simple and t["workspace"] != "none":
        ws_bytes = cb.scatter_workspace_bytes(dims, n, max(t["launch_samples"]), n_channels=max(planes, 1))
        if t["workspace"] == "short":
            ws_bytes = ws_bytes // 3
    use_carry = (not simple) and t["carry"] != "none"
    seq = Launches(cb, dims, n, planes=planes, seed=t["seed"], first=t["first"], workspace=ws_bytes, carry=use_carry or None)
    drain = {"drain_launch": "launch", "drain_flag": "flag"}[t["carry"]] if use_carry else None
    if fused:
        seq.launches(cb.draw_buddhabrot_channels, t["launch_samples"], variant | flags, drain=drain, windows=t["windows"])
    else:
        seq.launches(cb.draw_buddhabrot, t["launch_samples"], variant | flags, drain=drain,
                     iterations=cb.IterationControl(*(window or (t["max_iter"], t["min_iter"]))))
    return read(seq, on_device)[:2]


def anti_trial(rng):
    """An anti launch sequence: M at and around the product kernel's decisions (a round is 12 steps, a chunk 60, the
    first cycle can be found at 120), ragged thread counts, several launches on the same generators."""
    t = {}
    canvas_and_box(rng, t)
    t["ship"] = rng.random() < 0.3
    t["max_iter"] = rng.choice([0, 1, 5, 12, 59, 60, 61, 119, 120, 121, 180, 181, 240, 257, 360, 1000, 2000, 5000, 20000])
    t["threads"] = rng.choice([1, 63, 64, 65, 200, 256, 1000, 1024, 1337, 4096, 5000, 16384])
    if t["max_iter"] >= 5000:   # keep the lock-step kernel's run time in hand
        t["threads"] = min(t["threads"], 4096)
    t["launch_samples"] = [rng.choice([1, 2, 7, 50, 64, 100, 150]) for _ in range(rng.randint(1, 4))]
    t["seed"] = rng.choice([1337, 1337, 1, 0xdeadbeefcafe])
    t["first"] = rng.choice([0, 0, 1, 262144, 2097151])
    t["min_iter"] = rng.choice([0, 1, 20, 99, 1000, 30000])      # ignored by an anti launch
    t["buffers"] = rng.random() < 0.5                             # workspace and carry given (and ignored) or NULL
    return t


def render_anti(t, variant):
    """The launches of an anti trial -> (histogram, counters, generator states)."""
    dims = cb.FractalDimensions.make(t["w"], t["h"], *t["box"])
    n = t["threads"]
    flags = cb.CB_KERNEL_FLAG_ANTI | (cb.CB_KERNEL_FLAG_BURNING_SHIP if t["ship"] else 0)
    ws_bytes = max(cb.scatter_workspace_bytes(dims, n, max(t["launch_samples"])), 4096) if t["buffers"] else 0
    seq = Launches(cb, dims, n, seed=t["seed"], first=t["first"], workspace=ws_bytes, carry=t["buffers"] or None)
    return read(seq.launches(cb.draw_buddhabrot, t["launch_samples"], variant | flags, flush=False,  # nothing is deferred
                             iterations=cb.IterationControl(t["max_iter"], t["min_iter"])))


def power_trial(rng):
    """A Multibrot launch sequence: any degree, max_iter at and around the scheduler's rounds (12 steps) and chunks (60),
    ragged thread counts, several launches on the same generators, a plane out of unit rows or a random matrix."""
    t = {}
    canvas_and_box(rng, t)
    t["degree"] = rng.randint(cb.CB_POWER_MIN, cb.CB_POWER_MAX)
    t["max_iter"] = rng.choice([0, 1, 5, 11, 12, 13, 59, 60, 61, 119, 120, 121, 180, 257, 1000, 2000, 5000, 20000])
    t["min_iter"] = rng.choice([0, 0, 1, 2, 20, 59, 60, 99, 1000, 30000])
    t["threads"] = rng.choice([1, 63, 64, 65, 200, 256, 1000, 1024, 1337, 4096, 5000, 16384])
    if t["max_iter"] >= 5000:   # keep the lock-step kernel's run time in hand
        t["threads"] = min(t["threads"], 4096)
    t["launch_samples"] = [rng.choice([1, 2, 7, 50, 64, 100, 150]) for _ in range(rng.randint(1, 4))]
    t["seed"] = rng.choice([1337, 1337, 1, 0xdeadbeefcafe])
    t["first"] = rng.choice([0, 0, 1, 262144, 2097151])
    kind = rng.random()
    if kind < 0.3:
        t["matrix"] = list(cb.IDENTITY_PROJECTION)
    elif kind < 0.6:   # two different axes of (zr, zi, cr, ci)
        x, y = rng.sample(range(4), 2)
        t["matrix"] = [1.0 if j == x else 0.0 for j in range(4)] + [1.0 if j == y else 0.0 for j in range(4)]
    else:
        t["matrix"] = [rng.uniform(-1.5, 1.5) for _ in range(8)]
    return t


def render_power(t, variant):
    """The launches of a Multibrot trial -> (histogram, counters, generator states)."""
    seq = Launches(cb, cb.FractalDimensions.make(t["w"], t["h"], *t["box"]), t["threads"], seed=t["seed"], first=t["first"])
    return read(seq.launches(cb.draw_buddhabrot_projected, t["launch_samples"], variant | cb.CB_KERNEL_POWER(t["degree"]),
                             iterations=cb.IterationControl(t["max_iter"], t["min_iter"]), projection=t["matrix"]))


def depth_trial(rng):
    """A depth launch sequence: any step and either source of c, max_iter at and around the scheduler's rounds (12 steps)
    and chunks (60), ragged thread counts, several launches on the same generators, small canvases (the histogram is N
    of them), a plane and a depth row out of unit rows or random entries, a depth window that is dyadic or not, that
    holds everything, cuts the set or misses it."""
    t = {}
    t["w"] = rng.choice([1, 2, 7, 64, 100, 128, 129, 255, 256, 333])
    t["h"] = rng.choice([1, 3, 8, 64, 100, 127, 128, 200, 256])
    kind = rng.random()
    if kind < 0.5:
        t["box"] = (-2.0, 2.0, -2.0, 2.0)
    elif kind < 0.9:
        cx, cy = rng.uniform(-1.5, 0.5), rng.uniform(-1.0, 1.0)
        rx, ry = rng.uniform(0.05, 2.0), rng.uniform(0.05, 2.0)
        t["box"] = (cx - rx, cx + rx, cy - ry, cy + ry)
    else:
        t["box"] = (1.0, 3.0, 1.0, 2.5)
    step = rng.choice(["reference", "reference", "ship", "power", "formula"])
    t["degree"] = rng.randint(cb.CB_POWER_MIN, cb.CB_POWER_MAX) if step == "power" else 2
    t["ship"] = step == "ship"
    t["formula"] = rng.randint(cb.CB_FORMULA_TRICORN, cb.CB_FORMULA_MAX) if step == "formula" else 0
    t["c"] = None if rng.random() < 0.6 else (rng.choice([-0.8, 0.3, 0.0, -2.0, 2.0, rng.uniform(-2.0, 2.0)]),
                                              rng.choice([0.156, 0.0, 0.5, 2.0, rng.uniform(-2.0, 2.0)]))
    t["max_iter"] = rng.choice([0, 1, 5, 11, 12, 13, 59, 60, 61, 119, 120, 121, 180, 257, 500, 1000, 2000])
    t["min_iter"] = rng.choice([0, 0, 1, 2, 20, 59, 60, 99, 1000])
    t["threads"] = rng.choice([1, 63, 64, 65, 200, 256, 1000, 1024, 1337, 4096])
    if t["max_iter"] >= 1000:   # keep the lock-step kernel's run time in hand
        t["threads"] = min(t["threads"], 1024)
    t["launch_samples"] = [rng.choice([1, 2, 7, 50, 64]) for _ in range(rng.randint(1, 3))]
    t["seed"] = rng.choice([1337, 1337, 1, 0xdeadbeefcafe])
    t["first"] = rng.choice([0, 0, 1, 262144, 2097151])

    def unit(j):
        return [1.0 if k == j else 0.0 for k in range(4)]

    kind = rng.random()
    if kind < 0.3:
        t["matrix"] = list(cb.IDENTITY_PROJECTION)
    elif kind < 0.6:   # two different axes of (zr, zi, cr, ci)
        x, y = rng.sample(range(4), 2)
        t["matrix"] = unit(x) + unit(y)
    else:
        t["matrix"] = [rng.uniform(-1.5, 1.5) for _ in range(8)]
    t["row"] = unit(rng.randrange(4)) if rng.random() < 0.5 else [rng.uniform(-1.5, 1.5) for _ in range(4)]
    t["slices"] = rng.choice([1, 1, 2, 3, 4, 5, 7, 8, 16, 64, 100, 255, 256])
    kind = rng.random()
    if kind < 0.25:     # holds everything, dyadic for a power-of-two N
        t["window"] = (-64.0, 64.0)
    elif kind < 0.5:    # dyadic
        t["window"] = rng.choice([(-2.0, 2.0), (-1.0, 1.0), (-2.0, 0.0), (0.0, 0.5), (-0.125, 0.125)])
    elif kind < 0.9:    # anywhere near the set
        lo = rng.uniform(-2.5, 1.0)
        t["window"] = (lo, lo + rng.uniform(0.01, 3.0))
    else:               # far from it: almost nothing lands
        t["window"] = (5.0, 9.0)
    return t


def depth_palette_trial(rng):
    """A depth trial with a table of N entries in t["lut"]."""
    t = depth_trial(rng)
    n = t["slices"]
    kind = rng.random()
    if kind < 0.5:      # any weights, a third of the components zero
        lut = [sum((0 if rng.random() < 0.33 else rng.randint(1, 255)) << (8 * j) for j in range(3)) for _ in range(n)]
    elif kind < 0.65:   # one colour for every slice
        lut = [rng.choice([0x010101, 0x0000ff, 0xff00ff, 0x020100])] * n
    elif kind < 0.85:   # one slice lit
        lut = [0] * n
        lut[rng.randrange(n)] = rng.choice([1, 0x000100, 0x030201])
    else:               # small weights that differ from slice to slice
        lut = [(s % 3 + 1) | ((s * 7) % 5) << 8 | ((s >> 1) % 4) << 16 for s in range(n)]
    if rng.random() < 0.3:  # bits 24-31 are not read
        lut = [v | rng.randrange(256) << 24 for v in lut]
    t["lut"] = lut
    return t


def render_depth(t, variant):
    """The launches of a depth trial, or with t["lut"] of a depth-palette trial -> (histogram, counters, generator
    states)."""
    flags = ((cb.CB_KERNEL_POWER(t["degree"]) if t["degree"] != 2 else 0) | (cb.CB_KERNEL_FLAG_BURNING_SHIP if t["ship"] else 0)
             | (cb.CB_KERNEL_FORMULA(t["formula"]) if t["formula"] else 0))
    lut = t.get("lut")
    seq = Launches(cb, cb.FractalDimensions.make(t["w"], t["h"], *t["box"]), t["threads"], planes=3 if lut else t["slices"],
                   seed=t["seed"], first=t["first"], tables={"lut": lut} if lut else None)
    args = dict(iterations=cb.IterationControl(t["max_iter"], t["min_iter"]), projection=t["matrix"], julia_c=t["c"],
                depth=cb.Depth.make(t["row"], t["window"][0], t["window"][1], t["slices"]))
    if lut:
        args.update(d_lut=seq.tables["lut"].data_ptr(), n_entries=len(lut))
    entry = cb.draw_buddhabrot_depth_palette if lut else cb.draw_buddhabrot_depth
    return read(seq.launches(entry, t["launch_samples"], variant | flags, **args))


def frames_trial(rng):
    """A depth trial's step, source of c, canvas, window, iteration control, threads and launches, with F <= 16 matrices in
    t["frames"]: a rotation sweep of the trial's matrix, unit planes, random entries, or copies of one matrix."""
    t = depth_trial(rng)
    n = rng.choice([1, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16])
    kind = rng.random()
    if kind < 0.4:
        x, y = rng.sample(range(4), 2)
        lo = rng.choice([0.0, 0.0, -90.0, rng.uniform(-360.0, 360.0)])
        frames, _ = cb.frames_from_sweep(t["matrix"], (x, y), lo, lo + rng.choice([90.0, 360.0, rng.uniform(-400.0, 400.0)]), n)
        t["frames"] = [float(v) for v in frames.reshape(-1)]
    elif kind < 0.6:
        t["frames"] = []
        for _ in range(n):
            x, y = rng.sample(range(4), 2)
            t["frames"] += [1.0 if k == x else 0.0 for k in range(4)] + [1.0 if k == y else 0.0 for k in range(4)]
    elif kind < 0.85:
        t["frames"] = [rng.uniform(-1.5, 1.5) for _ in range(8 * n)]
    else:
        t["frames"] = list(t["matrix"]) * n
    for k in ("matrix", "row", "slices", "window"):
        del t[k]
    return t


def render_frames(t, variant):
    """The launches of a frames trial -> (histogram, counters, generator states)."""
    flags = ((cb.CB_KERNEL_POWER(t["degree"]) if t["degree"] != 2 else 0) | (cb.CB_KERNEL_FLAG_BURNING_SHIP if t["ship"] else 0)
             | (cb.CB_KERNEL_FORMULA(t["formula"]) if t["formula"] else 0))
    n = len(t["frames"]) // 8
    seq = Launches(cb, cb.FractalDimensions.make(t["w"], t["h"], *t["box"]), t["threads"], planes=n, seed=t["seed"],
                   first=t["first"])
    d_frames = seq.on_device(np.array(t["frames"], dtype=np.float64).view(np.uint64), np.uint64)  # alive to the read
    out = read(seq.launches(cb.draw_buddhabrot_frames, t["launch_samples"], variant | flags,
                            iterations=cb.IterationControl(t["max_iter"], t["min_iter"]), d_frames=d_frames.data_ptr(),
                            n_frames=n, julia_c=t["c"]))
    del d_frames
    return out


def phoenix_trial(rng):
    """A depth trial's source of c, canvas, window, matrix, iteration control, threads and launches, with a parameter p in
    t["p"]; the step is the render's own."""
    t = depth_trial(rng)
    kind = rng.random()
    if kind < 0.15:
        t["p"] = (0.0, 0.0)
    elif kind < 0.45:   # real p: with a real c and z_0 the Henon map
        t["p"] = (rng.choice([-0.5, 0.25, 0.3, -1.0, rng.uniform(-1.0, 1.0)]), 0.0)
    elif kind < 0.55:   # the ends of the range
        t["p"] = (rng.choice([-2.0, 2.0]), rng.choice([-2.0, 0.0, 2.0]))
    else:
        t["p"] = (rng.uniform(-1.0, 1.0), rng.uniform(-1.0, 1.0)) if rng.random() < 0.7 else (rng.uniform(-2.0, 2.0),
                                                                                            rng.uniform(-2.0, 2.0))
    for k in ("degree", "ship", "formula", "row", "slices", "window"):
        del t[k]
    return t


def render_phoenix(t, variant):
    """The launches of a Phoenix trial -> (histogram, counters, generator states)."""
    seq = Launches(cb, cb.FractalDimensions.make(t["w"], t["h"], *t["box"]), t["threads"], seed=t["seed"], first=t["first"])
    return read(seq.launches(cb.draw_buddhabrot_phoenix, t["launch_samples"], variant,
                             iterations=cb.IterationControl(t["max_iter"], t["min_iter"]), projection=t["matrix"],
                             julia_c=t["c"], phoenix_p=t["p"]))


def periods_trial(rng):
    """A depth trial's step, source of c, canvas, window, matrix, iteration control, threads and launches, with a table of
    2 .. CB_PERIOD_MAX_ENTRIES entries in t["lut"] and a tolerance in t["eps"]."""
    t = depth_trial(rng)
    for k in ("row", "slices", "window"):
        del t[k]
    n = rng.choice([2, 2, 3, 4, 13, 60, 61, 62, 256, cb.CB_PERIOD_MAX_ENTRIES, rng.randint(2, cb.CB_PERIOD_MAX_ENTRIES)])
    if t["max_iter"] >= 1000:   # keep the lock-step kernel's run time in hand: its search is up to n - 1 steps per orbit
        n = min(n, 256)
    kind = rng.random()
    if kind < 0.5:      # any weights, a third of the components zero
        lut = [sum((0 if rng.random() < 0.33 else rng.randint(1, 255)) << (8 * j) for j in range(3)) for _ in range(n)]
    elif kind < 0.65:   # one colour for every period
        lut = [rng.choice([0x010101, 0x0000ff, 0xff00ff, 0x020100])] * n
    elif kind < 0.85:   # one period lit: every other orbit is not replayed
        lut = [0] * n
        lut[rng.choice([0, 1, 1, rng.randrange(n)])] = rng.choice([1, 0x000100, 0x030201])
    else:               # small weights that differ from period to period
        lut = [(s % 3 + 1) | ((s * 7) % 5) << 8 | ((s >> 1) % 4) << 16 for s in range(n)]
    if rng.random() < 0.3:  # bits 24-31 are not read
        lut = [v | rng.randrange(256) << 24 for v in lut]
    t["lut"] = lut
    t["eps"] = rng.choice([0.0, 2.0 ** -66, 2.0 ** -66, 1e-20, 2.0 ** -30, 1e-3, 2.0 ** 10])
    return t


def render_periods(t, variant):
    """The launches of a period-palette trial -> (planes, counters, generator states)."""
    flags = ((cb.CB_KERNEL_POWER(t["degree"]) if t["degree"] != 2 else 0) | (cb.CB_KERNEL_FLAG_BURNING_SHIP if t["ship"] else 0)
             | (cb.CB_KERNEL_FORMULA(t["formula"]) if t["formula"] else 0))
    seq = Launches(cb, cb.FractalDimensions.make(t["w"], t["h"], *t["box"]), t["threads"], planes=3, seed=t["seed"],
                   first=t["first"], tables={"lut": t["lut"]})
    return read(seq.launches(cb.draw_buddhabrot_periods, t["launch_samples"], variant | flags,
                             iterations=cb.IterationControl(t["max_iter"], t["min_iter"]), projection=t["matrix"],
                             julia_c=t["c"], d_lut=seq.tables["lut"].data_ptr(), n_entries=len(t["lut"]),
                             period_eps=t["eps"]))


def sums_up(want, wc):
    return int(want.sum()) == wc["increments"]


# One row per mode of the lock-step / product A/B that compares generator states as well: the trial generator and its
# render; the values of cb_debug_last_draw_kernel (lock-step, product); `extra`, what else the lock-step run must satisfy
# -- (wanted histogram, its counters) -> bool -- and what a MISMATCH block says about it (counters_note, pixels_note); and
# `filled`: the final line also tallies the trials with increments > 0.
AB_MODES = {
    "ANTI": dict(name="anti", trial=anti_trial, render=render_anti, kernels=(5, 4)),
    "POWER": dict(name="power", trial=power_trial, render=render_power, kernels=(11, 10),
                  extra=lambda want, wc: wc["rejected"] == 0, counters_note=", rejected %(rejected)d"),
    "DEPTH": dict(name="depth", trial=depth_trial, render=render_depth, kernels=(19, 18), extra=sums_up,
                  pixels_note="; increments %(increments)d", filled=True),
    "DEPTHPALETTE": dict(name="depth-palette", trial=depth_palette_trial, render=render_depth, kernels=(21, 20),
                         extra=sums_up, pixels_note="; increments %(increments)d", filled=True),
    "FRAMES": dict(name="frames", trial=frames_trial, render=render_frames, kernels=(23, 22), extra=sums_up,
                   pixels_note="; increments %(increments)d", filled=True),
    "PHOENIX": dict(name="phoenix", trial=phoenix_trial, render=render_phoenix, kernels=(25, 24),
                    extra=lambda want, wc: sums_up(want, wc) and wc["rejected"] == 0,
                    counters_note=", rejected %(rejected)d", pixels_note="; increments %(increments)d", filled=True),
    "PERIODS": dict(name="periods", trial=periods_trial, render=render_periods, kernels=(29, 28),
                    extra=lambda want, wc: sums_up(want, wc) and wc["rejected"] == 0,
                    counters_note=", rejected %(rejected)d", pixels_note="; increments %(increments)d", filled=True),
}


def ab_main(mode, seconds, seed):
    """One mode of AB_MODES until SECONDS have passed, or TRIALS trials where that comes first."""
    name, render_mode, (lockstep_kernel, product_kernel) = mode["name"], mode["render"], mode["kernels"]
    rng = random.Random(seed)
    t_end = time.time() + seconds
    trials = int(os.environ.get("TRIALS", "0"))
    n = early = filled = 0
    last_print = time.time()
    while time.time() < t_end and not (trials and n >= trials):
        t = mode["trial"](rng)
        try:
            want, wc, want_states = render_mode(t, cb.CB_KERNEL_SIMPLE)
            lockstep_ran = cb.lib.cb_debug_last_draw_kernel() == lockstep_kernel
            got, gc, got_states = render_mode(t, cb.CB_KERNEL_DEFAULT)
            product_ran = cb.lib.cb_debug_last_draw_kernel() == product_kernel
        except cb.CudabrotError as e:
            print("trial %d: error %s\n  %r" % (n, e, t), flush=True)
            return 1
        bad = [k for k in COMPARED if wc[k] != gc[k]]
        if not np.array_equal(want, got) or bad or not np.array_equal(want_states, got_states) or not (
                lockstep_ran and product_ran) or wc["skipped_steps"] != 0 or (
                "extra" in mode and not mode["extra"](want, wc)):
            print("MISMATCH at %s trial %d (seed %d): %r" % (name, n, seed, t))
            print("  kernels as expected: lock-step %s, product %s" % (lockstep_ran, product_ran))
            print("  counters that differ: %r; lock-step skipped_steps %d%s" % (
                [(k, wc[k], gc[k]) for k in bad], wc["skipped_steps"], mode.get("counters_note", "") % wc))
            print("  generator states identical: %s" % np.array_equal(want_states, got_states))
            print("  pixels that differ: %d of %d; sums %d vs %d%s" % (
                int((want != got).sum()), want.size, int(want.sum()), int(got.sum()), mode.get("pixels_note", "") % wc),
                flush=True)
            return 1
        n += 1
        early += 1 if gc["skipped_steps"] > 0 else 0
        filled += 1 if wc["increments"] > 0 else 0
        if time.time() - last_print > 30:
            print("%d %s trials identical so far (%d with skipped_steps > 0)" % (n, name, early), flush=True)
            last_print = time.time()
    tallies = "%d with skipped_steps > 0" % early + (", %d with increments > 0" % filled if mode.get("filled") else "")
    print("gpu_fuzz: %d %s trials (%s), histograms, counters and generator states identical (seed %d)" % (
        n, name, tallies, seed))
    return 0


def heavy_trial(rng):
    """Product-sized launches: the deferred scatter (one and two sort levels, carry) against the same
    kernel with direct atomics -- the lock-step kernel would take minutes at these sizes."""
    t = trial(rng)
    t["w"] = rng.choice([1000, 4096, 6000, 9000, 12000])
    t["h"] = rng.choice([1000, 4096, 6000, 9000])
    if rng.random() < 0.6:
        t["box"] = (-2.0, 2.0, -2.0, 2.0)
    t["max_iter"] = rng.choice([100, 2000, 20000])
    t["min_iter"] = rng.choice([0, 20, 20, 40])
    t["threads"] = rng.choice([65536, 100000, 262144])
    t["launch_samples"] = [rng.choice([50, 100, 400]) for _ in range(rng.randint(1, 3))]
    t["workspace"] = rng.choice(["suggested", "suggested", "short"])
    t["windows"] = None
    t["heavy"] = True
    return t


def renderer_trial(rng):
    """The owned-object form (cb_renderer: two workspaces and streams, carry, lazy drain, resume)."""
    t = trial(rng)
    t["threads"] = rng.choice([64, 200, 1024, 4096])
    t["max_iter"] = min(t["max_iter"], 2000)
    t["calls"] = [rng.choice([1, 2, 3, 7, 64, 70]) for _ in range(rng.randint(1, 3))]
    if sum(t["calls"]) > 80:
        t["calls"] = [3, 66]
    t["per_launch"] = rng.choice([None, 1, 2, 5, 64])
    t["no_workspace"] = rng.random() < 0.2
    t["read_between"] = rng.random() < 0.3       # reading the histogram drains the carried orbits early
    t["resume_at"] = rng.choice([None, None, 0, 1])   # after this call: states + histogram into a NEW renderer
    t["launch_samples"] = [50 * sum(t["calls"])]
    return t


def render_with_renderer(t):
    for k, v in (("CUDABROT_AMD_PASSES_PER_LAUNCH", t["per_launch"]), ("CUDABROT_AMD_NO_WORKSPACE", 1 if t["no_workspace"] else None),
                 ("CUDABROT_AMD_TWO_LEVEL", 1 if t["two_level"] else None),
                 ("CUDABROT_AMD_CHUNKED", 1 if t.get("chunked", True) else 0)):
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    dims = cb.FractalDimensions.make(t["w"], t["h"], *t["box"])
    what = t["windows"] if t["windows"] else cb.IterationControl(t["max_iter"], t["min_iter"])
    flags = cb.CB_KERNEL_FLAG_BURNING_SHIP if t["ship"] else 0
    r = cb.Renderer(dims, what, seed=t["seed"], first_subsequence=t["first"], n_threads=t["threads"])
    try:
        for i, passes in enumerate(t["calls"]):
            r.render_passes(passes, cb.CB_KERNEL_DEFAULT | flags)
            if t["read_between"]:
                r.read_histogram()
            if t["resume_at"] == i:
                hist, states = r.read_histogram(), r.read_rng_states()
                r.close()
                r = cb.Renderer(dims, what, seed=99, first_subsequence=5, n_threads=t["threads"])
                r.write_histogram(hist)
                r.write_rng_states(states)
        hist = r.read_histogram().reshape(-1)
        status = r.read_counters().status
    finally:
        r.close()
        for k in ("CUDABROT_AMD_PASSES_PER_LAUNCH", "CUDABROT_AMD_NO_WORKSPACE", "CUDABROT_AMD_TWO_LEVEL"):
            os.environ.pop(k, None)
    return hist, int(status)


def main():
    seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    for knob, mode in AB_MODES.items():
        if os.environ.get(knob) == "1":
            return ab_main(mode, seconds, seed)
    rng = random.Random(seed)
    t_end = time.time() + seconds
    n = 0
    last_print = time.time()
    wide_trials = [0]   # trials whose last product launch was draw_wide_kernel's
    while time.time() < t_end:
        if os.environ.get("HEAVY") == "1":
            t = heavy_trial(rng)
        else:
            t = renderer_trial(rng) if rng.random() < 0.3 else trial(rng)
        try:
            if "heavy" in t:
                got_d, gc = render(t, cb.CB_KERNEL_DEFAULT, on_device=True)
                if cb.lib.cb_debug_last_draw_kernel() == 2:
                    wide_trials[0] += 1
                direct = dict(t, workspace="none", carry="none", two_level=False)
                want_d, wc = render(direct, cb.CB_KERNEL_DEFAULT, on_device=True)
                same = bool(torch.equal(got_d, want_d))
                want, got = (np.zeros(1), np.zeros(1)) if same else (want_d.cpu().numpy(), got_d.cpu().numpy())
                del got_d, want_d
            elif "calls" in t:
                got, status = render_with_renderer(t)
                t["two_level"] = False
                if t["windows"]:
                    want = np.concatenate([render(t, cb.CB_KERNEL_SIMPLE, window=w)[0] for w in t["windows"]])
                else:
                    want = render(t, cb.CB_KERNEL_SIMPLE)[0]
                wc = gc = {k: 0 for k in COMPARED}
                gc = dict(gc, status=status)
            elif t["windows"]:
                got, gc = render(t, cb.CB_KERNEL_DEFAULT, fused=True)
                singles = [render(t, cb.CB_KERNEL_SIMPLE, window=w) for w in t["windows"]]
                want = np.concatenate([h for h, _ in singles])
                # per-window counters do not add up to the fused run's: what one run with the largest max and the smallest
                # min counts is taken from a lock-step run of that window, the increments from the windows' runs, and
                # too_fast, recorded and replay_steps stay the fused run's own
                hull = (max(m for m, _ in t["windows"]), min(c for _, c in t["windows"]))
                of_hull = render(t, cb.CB_KERNEL_SIMPLE, window=hull)[1]
                wc = dict(gc)
                for k in ("samples", "rejected", "never_escaped", "iterate_steps"):
                    wc[k] = of_hull[k]
                wc["increments"] = sum(c["increments"] for _, c in singles)
            else:
                want, wc = render(t, cb.CB_KERNEL_SIMPLE)
                got, gc = render(t, cb.CB_KERNEL_DEFAULT)
                if cb.lib.cb_debug_last_draw_kernel() == 2:
                    wide_trials[0] += 1
        except cb.CudabrotError as e:
            print("trial %d: error %s\n  %r" % (n, e, t), flush=True)
            return 1
        bad = [k for k in COMPARED if wc[k] != gc[k]]
        if not np.array_equal(want, got) or bad:
            print("MISMATCH at trial %d (seed %d): %r" % (n, seed, t))
            print("  counters that differ: %r" % [(k, wc[k], gc[k]) for k in bad])
            print("  pixels that differ: %d of %d; sums %d vs %d" % (int((want != got).sum()), want.size,
                                                                     int(want.sum()), int(got.sum())), flush=True)
            return 1
        n += 1
        if "heavy" in t:
            print("  ok: %dx%d max_iter %d threads %d samples %r ws %s carry %s two_level %s" % (
                t["w"], t["h"], t["max_iter"], t["threads"], t["launch_samples"], t["workspace"], t["carry"],
                t["two_level"] or (t["w"] + 127) // 128 * ((t["h"] + 127) // 128) > 4096), flush=True)
        if time.time() - last_print > 30:
            print("%d trials identical so far (%d through draw_wide_kernel)" % (n, wide_trials[0]), flush=True)
            last_print = time.time()
    print("gpu_fuzz: %d trials (%d through draw_wide_kernel), histograms and counters identical (seed %d)" % (n, wide_trials[0], seed))
    return 0


if __name__ == "__main__":
    sys.exit(main())
