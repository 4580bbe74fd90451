"""Throughput of the render families through cb_renderer (method in section 7): one tool, one method,
one record.

    python tools/render_rate.py FAMILY [options]       FAMILY: anti focus project power julia palette formula depth
    python tools/render_rate.py FAMILY [options] --list         depth_palette frames phoenix
    python tools/render_rate.py --one '<case as JSON>'

A family is a list of cases; a case is plain data that says everything about one measurement.  Every case is measured in
a process of its own under its own time limit (--limit), a child of this script started with --one: a renderer
configured from the case, prepare, one warm-up pass, then --reps repetitions of whole batches of passes until --seconds
have passed, finish() included.  The child prints one JSON line: the case, `kernel` (cb_debug_last_draw_kernel after the
warm-up), `status`, the lists `passes`, `ms_per_pass` and `msamples_per_s` (one entry per repetition) with their medians,
and from the counters of all repetitions `executed_steps_per_sample` (iterate + replay - skipped), `counted_steps_per_sample`
(iterate + replay), `increments_per_sample`, `mincrements_per_s` and `never_escaped_fraction`.  The first child that
fails, dies or runs out of time ends the script with that status: nothing more is started on the device after it.
--list prints the cases and touches neither the library nor a device.
"""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]
C_JULIA = [-0.8, 0.156]
FORMULA_ROWS = ("ship", "tricorn", "celtic", "buffalo", "perpendicular", "celtic-tricorn", "lockstep")
DEPTH_PALETTE_KINDS = {"depth": "depth product", "palette": "depth-palette product", "lockstep": "depth-palette lock-step"}
# name -> (fixed c, p or None for the Julia render itself, lock-step)
PHOENIX_RENDERS = {
    "phoenix": (None, [-0.5, 0.0], False),
    "phoenix_p0": (None, [0.0, 0.0], False),
    "julia": (C_JULIA, None, False),
    "phoenix_julia": (C_JULIA, [0.0, 0.0], False),
    "lockstep": (None, [-0.5, 0.0], True),
}
COUNTERS = ("samples", "never_escaped", "iterate_steps", "replay_steps", "skipped_steps", "increments")


def case(a, what, max_iter, lockstep=False, **fields):
    """One measurement.  The kernel variant: lockstep, anti, ship, power (a degree), formula (a name).  The renderer's
    setup: box, projection, julia (c), phoenix (p), depth (row, min, max, N) -- with depth_palette as the table's slices
    --, palette_planes (the non-zero planes of the table), sweep (F frames of zi,cr:0:90:F), focus (level, probe,
    dilate); none of them is the normal render.  separate: not one render with F frames but F renders, one per matrix
    of the sweep, their times per pass summed."""
    c = {"family": a.family, "what": what, "max_iter": max_iter, "min_iter": a.c, "side": a.side, "box": None,
         "lockstep": bool(lockstep), "anti": False, "ship": False, "power": 0, "formula": None,
         "projection": None, "julia": None, "phoenix": None, "depth": None, "depth_palette": False, "palette_planes": 0,
         "sweep": 0, "separate": False, "focus": None,
         "batch": 1 if lockstep else 4, "max_batches": 4 if lockstep else 64,
         "seconds": a.seconds, "reps": a.reps, "threads": a.threads}
    assert set(fields) <= set(c), fields
    c.update(fields)
    return c


def ints(text):
    return [int(v) for v in text.split(",")]


def pair(text, sep=","):
    """'RE,IM' -> [re, im]; 'none' -> None."""
    return None if text == "none" else [float(v) for v in text.split(sep)]


def anti(a):
    return [case(a, "anti lock-step" if k else "anti product", m, k, anti=True) for m in ints(a.max_iters) for k in (0, 1)]


def focus(a):
    box = [float(x) for x in a.box.split(",")]
    f = {"level": a.level, "probe": a.probe, "dilate": a.dilate}
    return [case(a, "normal", a.m, box=box, batch=128, max_batches=64),
            case(a, "focus product", a.m, box=box, focus=f),
            case(a, "focus lock-step", a.m, 1, box=box, focus=f, batch=a.lockstep_batch)]


def project(a):
    rows = a.project.split(":")
    p = [float.fromhex(x) if "0x" in x.lower() else float(x) for row in rows for x in row.split(",")]
    if len(rows) != 2 or len(p) != 8:
        raise ValueError("--project wants a,b,c,d:e,f,g,h")
    return ([] if a.skip_normal else [case(a, "normal", a.m, batch=128, max_batches=64)]) + \
        [case(a, "project product", a.m, projection=p)] + \
        ([] if a.skip_lockstep else [case(a, "project lock-step", a.m, 1, projection=p)])


def power(a):
    return [case(a, "power lock-step" if k else "power product", m, k, power=d, projection=IDENTITY)
            for m in ints(a.max_iters) for d in ints(a.degrees) for k in (0, 1)]


def plotted(c):
    """The setup of a plotted render on the identity plane: a fixed c, or a sampled one."""
    return {"projection": IDENTITY} if c is None else {"julia": c}


def julia(a):
    return [case(a, ("projected" if c is None else "julia") + (" lock-step" if k else " product"), m, k, **plotted(c))
            for m in ints(a.max_iters) for c in map(pair, a.cs.split(":")) for k in ((0,) if c is None else (0, 1))]


def palette(a):
    c = pair(a.julia)
    return [case(a, ("julia" if c else "projected") + (" palette, %d plane(s)" % n if n else ", no palette"), a.max_iter,
                 palette_planes=n, **plotted(c)) for n in ints(a.planes)]


def formula(a):
    rows = a.rows.split(",")
    if any(row not in FORMULA_ROWS for row in rows):
        raise ValueError("--rows takes " + ", ".join(FORMULA_ROWS))
    return [case(a, row, a.m, row == "lockstep", projection=IDENTITY, ship=row == "ship",
                 formula={"ship": None, "lockstep": "tricorn"}.get(row, row)) for row in rows]


def depth(a):
    lo, hi = pair(a.window, ":")
    # the projected render's product kernel first, then each slice count, product and lock-step
    return [c for m in ints(a.max_iters) for c in [case(a, "projected product", m, projection=IDENTITY)] + [
        case(a, "depth lock-step" if k else "depth product", m, k, projection=IDENTITY, depth=["cr", lo, hi, n])
        for n in ints(a.slices) for k in (0, 1)]]


def depth_palette(a):
    lo, hi = pair(a.window, ":")
    kinds = a.kinds.split(",")
    if any(k not in DEPTH_PALETTE_KINDS for k in kinds):
        raise ValueError("--kinds takes " + ", ".join(DEPTH_PALETTE_KINDS))
    return [case(a, DEPTH_PALETTE_KINDS[k], m, k == "lockstep", projection=IDENTITY, depth=["cr", lo, hi, n],
                 depth_palette=k != "depth") for m in ints(a.max_iters) for n in ints(a.slices) for k in kinds]


def frames(a):
    return [case(a, "%d separate renders" % n if sep else "frames render", a.m, projection=IDENTITY, sweep=n, separate=sep,
                 julia=C_JULIA if src == "julia" else None, seconds=a.plain_seconds if sep else a.seconds)
            for src in a.sources.split(",") for n in ints(a.frames) for sep in (False, True)]


def phoenix(a):
    out = []
    for m in ints(a.m):
        for name in a.renders.split(","):
            c, p, lockstep = PHOENIX_RENDERS[name]
            out.append(case(a, name, m, lockstep, phoenix=p, max_batches=16 if lockstep else 64, **plotted(c)))
    return out


COMMON = {"-c": 20, "--side": 4096, "--seconds": 0.5, "--reps": 3, "--limit": 120.0}
# family -> (args -> cases, its own options and the defaults it changes)
FAMILIES = {
    "anti": (anti, {"--max-iters": "500,20000"}),
    "focus": (focus, {"--box": "-0.2,0.0,-0.9,-0.7", "-m": 20000, "--level": 8, "--probe": 64, "--dilate": 1,
                      "--lockstep-batch": 1}),
    "project": (project, {"-m": 20000, "--project": "1,0,0,0:0,1,0,0", "--skip-normal": False, "--skip-lockstep": False}),
    "power": (power, {"--degrees": "3,8", "--max-iters": "500,20000"}),
    "julia": (julia, {"--cs": "-1,0:-0.8,0.156:none", "--max-iters": "20000"}),
    "palette": (palette, {"--planes": "0,1,2,3", "--max-iter": 2000, "--julia": "none"}),
    "formula": (formula, {"--rows": ",".join(FORMULA_ROWS), "-m": 2000}),
    "depth": (depth, {"--slices": "1,64", "--max-iters": "500,20000", "--window": "-2:0.5"}),
    "depth_palette": (depth_palette, {"--slices": "64,256", "--max-iters": "500,20000", "--window": "-2:2",
                                      "--kinds": ",".join(DEPTH_PALETTE_KINDS)}),
    "frames": (frames, {"--frames": "1,8,64", "--sources": "sampled,julia", "-m": 2000, "--plain-seconds": 0.5,
                        "--side": 1024, "--limit": 240.0}),
    "phoenix": (phoenix, {"--renders": ",".join(PHOENIX_RENDERS), "-m": "500,2000", "--limit": 240.0}),
}


def timed(cb, case):
    """One renderer configured from the case: warm-up pass, then case["reps"] repetitions of whole batches for at least
    case["seconds"] -> kernel, status, the focus probe's figures and per repetition (seconds, passes, counters delta)."""
    import numpy as np

    kernel = ((cb.CB_KERNEL_SIMPLE if case["lockstep"] else cb.CB_KERNEL_DEFAULT)
              | (cb.CB_KERNEL_FLAG_ANTI if case["anti"] else 0) | (cb.CB_KERNEL_FLAG_BURNING_SHIP if case["ship"] else 0)
              | (cb.CB_KERNEL_POWER(case["power"]) if case["power"] else 0)
              | (cb.CB_KERNEL_FORMULA(case["formula"]) if case["formula"] else 0))
    dims = cb.FractalDimensions.make(case["side"], case["side"], *(case["box"] or ()))
    batch, out = case["batch"], {"probe_seconds": 0.0, "cells": 0, "cells_total": 0, "reps": []}
    with cb.Renderer(dims, cb.IterationControl(case["max_iter"], case["min_iter"]), device=0,
                     n_threads=case["threads"] or cb.CB_DEFAULT_THREADS) as r:
        if case["focus"]:
            t0 = time.perf_counter()
            out["cells"], out["cells_total"] = r.set_focus(case["focus"]["level"], case["focus"]["probe"],
                                                           case["focus"]["dilate"], kernel)
            out["probe_seconds"] = round(time.perf_counter() - t0, 4)
        if case["julia"]:
            r.set_julia(case["julia"], case["projection"])
        elif case["projection"]:
            r.set_projection(case["projection"])
        if case["phoenix"]:
            r.set_phoenix(case["phoenix"])
        if case["palette_planes"]:  # R = 1 / R = G = 1 / R = G = B = 1 for every k: one, two or three atomics a point
            r.set_palette(np.full(case["max_iter"], (0x010101 >> (8 * (3 - case["palette_planes"]))), dtype=np.uint32))
        if case["depth_palette"]:  # dark blue to orange to white: no weight is zero anywhere
            slices = case["depth"][3]
            last = max(slices - 1, 1)
            lut = cb.palette_from_stops([(0, 0x01, 0x02, 0x30), (last // 2 if last > 1 else 0, 0xFF, 0x80, 0x01),
                                         (last, 0xFF, 0xFF, 0xFF)][0 if last > 1 else 1:], slices)
            assert all((int(v) >> s) & 0xFF for v in lut for s in (0, 8, 16))
            r.set_depth_palette(case["depth"], lut)
        elif case["depth"]:
            r.set_depth(case["depth"])
        if case["sweep"]:
            r.set_frames(cb.frames_from_sweep(case["projection"], ("zi", "cr"), 0.0, 90.0, case["sweep"])[0])
        r.prepare(kernel)
        r.render_passes(1, kernel)  # warm-up: code objects, the interior map, first touch of the histogram
        r.finish()
        out["kernel"] = cb.lib.cb_debug_last_draw_kernel()
        for _ in range(case["reps"]):
            before = r.read_counters().as_dict()
            passes = 0
            t0 = time.perf_counter()
            while True:  # whole batches until the time asked for has passed
                r.render_passes(batch, kernel)
                r.finish()
                passes += batch
                dt = time.perf_counter() - t0
                if dt >= case["seconds"] or passes >= case["max_batches"] * batch:
                    break
            after = r.read_counters().as_dict()
            out["reps"].append((dt, passes, {k: after[k] - before[k] for k in COUNTERS}))
        out["status"] = r.read_counters().as_dict()["status"]
    return out


def measure(case):
    """The record of one case (the module's docstring names its keys)."""
    sys.path.insert(0, ROOT)
    import cudabrot_amd as cb

    parts = [case]
    if case["separate"]:  # a renderer of its own per frame: what F runs with --rotate do
        mats = cb.frames_from_sweep(case["projection"], ("zi", "cr"), 0.0, 90.0, case["sweep"])[0]
        parts = [dict(case, projection=[float(x) for x in p], sweep=0) for p in mats]
    runs = [timed(cb, p) for p in parts]
    reps = list(zip(*[run["reps"] for run in runs]))  # per repetition: every part's (seconds, passes, counters delta)
    rec = dict(case, kernel=runs[-1]["kernel"], status=0)
    for run in runs:
        rec["status"] |= run["status"]
    rec["passes"] = [sum(n for _, n, _ in rep) for rep in reps]
    rec["ms_per_pass"] = [round(sum(1e3 * dt / n for dt, n, _ in rep), 3) for rep in reps]
    rec["msamples_per_s"] = [round(sum(d["samples"] for _, _, d in rep) / sum(dt for dt, _, _ in rep) / 1e6, 2) for rep in reps]
    for k in ("passes", "ms_per_pass", "msamples_per_s"):
        rec["median_" + k] = statistics.median(rec[k])
    if case["separate"]:
        each = [round(statistics.median(1e3 * dt / n for dt, n, _ in run["reps"]), 3) for run in runs]
        rec["each_ms"] = each if len(each) <= 8 else [min(each), max(each)]
    seconds = sum(dt for rep in reps for dt, _, _ in rep)
    d = {k: sum(delta[k] for rep in reps for _, _, delta in rep) for k in COUNTERS}
    counted = d["iterate_steps"] + d["replay_steps"]
    rec.update(executed_steps_per_sample=round((counted - d["skipped_steps"]) / d["samples"], 2),
               counted_steps_per_sample=round(counted / d["samples"], 2),
               increments_per_sample=round(d["increments"] / d["samples"], 6),
               mincrements_per_s=round(d["increments"] / seconds / 1e6, 3),
               never_escaped_fraction=round(d["never_escaped"] / d["samples"], 5))
    if case["focus"]:
        rec.update({k: runs[0][k] for k in ("probe_seconds", "cells", "cells_total")})
    return rec


def run_children(commands, limit):
    """Start each (label, argv) as a fresh process under `limit` seconds, one after another -> 0, or the status of the
    first that fails (128 + the signal it died on; 124: it ran past the limit).  Nothing is started after that one."""
    for label, argv in commands:
        try:
            rc = subprocess.run(argv, timeout=limit).returncode
        except subprocess.TimeoutExpired:
            print("render_rate: %s ran past %g s: stopping" % (label, limit), flush=True)
            return 124
        if rc != 0:
            print("render_rate: %s ended with status %d: stopping" % (label, rc), flush=True)
            return rc if rc > 0 else 128 - rc
    return 0


def label(case):
    return "%s: %s, -m %d" % (case["family"], case["what"], case["max_iter"])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--one", metavar="CASE", help="(a child: measure this case, given as JSON)")
    sub = ap.add_subparsers(dest="family", metavar="FAMILY")
    for name, (_, own) in FAMILIES.items():
        p = sub.add_parser(name)
        for flag, default in {**COMMON, **own}.items():
            if default is False:
                p.add_argument(flag, action="store_true")
            else:
                p.add_argument(flag, type=type(default), default=default)
        p.add_argument("--threads", type=int, help="threads of the renderer (default: CB_DEFAULT_THREADS)")
        p.add_argument("--list", action="store_true", help="print the cases, one JSON line each, and exit")
    a = ap.parse_args(argv)
    if a.one:
        print(json.dumps(measure(json.loads(a.one))), flush=True)
        return 0
    if not a.family:
        ap.error("a FAMILY, or --one CASE")
    try:
        cases = FAMILIES[a.family][0](a)
    except (ValueError, KeyError) as e:
        ap.error(str(e))
    if a.list:
        for c in cases:
            print(json.dumps(c))
        return 0
    return run_children([(label(c), [sys.executable, os.path.abspath(__file__), "--one", json.dumps(c)]) for c in cases],
                        a.limit)


if __name__ == "__main__":
    sys.exit(main())
