#!/usr/bin/env python3
"""Times the white clip on real renders, on a GPU (the record is profiles/exposure_rate.txt).

usage: exposure_rate.py PKGROOT {current|parent} OUT.jsonl [SIZE...]

PKGROOT is the directory that holds the cudabrot_amd package to load: this tree, or a build of another commit to time its
unclipped image call beside this one's (`parent`: only that call is timed).  For every SIZE a SIZE x SIZE canvas is rendered
(1000 / 20 iterations, 64 passes up to 4096, 32 above) and, three repetitions each by the host clock around calls that end
in a device synchronise: cb_renderer_grayscale_image without a clip; cb_white_count_device at p = 0.1 (every pass) and at
p = 0 (pass 0 alone), from which the bytes per second of pass 0 and of a digit pass follow; the image call with the clip;
the unclipped call again.  `current` then makes README.md's two --bounded renders at 4096 x 4096 for about 12 s each and
says what their images hold with and without --white-clip 0.1.  One JSON line per figure, appended to OUT.jsonl."""
import json
import statistics
import sys
import time

pkgroot, which, out_path = sys.argv[1:4]
sizes = [int(s) for s in sys.argv[4:]]
sys.path.insert(0, pkgroot)
import numpy as np  # noqa: E402

import cudabrot_amd as cb  # noqa: E402

assert cb.library_path().startswith(pkgroot), cb.library_path()
out = open(out_path, "a")


def say(**kw):
    kw["which"] = which
    line = json.dumps(kw)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def timed(f, reps=3):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts)}


for size in sizes:
    dims = cb.FractalDimensions.make(size, size)
    passes = 64 if size <= 4096 else 32
    with cb.Renderer(dims, cb.IterationControl(1000, 20)) as r:
        t0 = time.perf_counter()
        r.render_passes(passes)
        r.finish()
        say(size=size, what="render", passes=passes, seconds=time.perf_counter() - t0)
        n = size * size
        r.grayscale_image(2.2)  # warm
        say(size=size, what="grayscale_image unclipped", **timed(lambda: r.grayscale_image(2.2)))
        if which == "current":
            ptr = r.device_histogram
            cb.white_count_device(ptr, n, 0.1)
            white, lit, clipped = cb.white_count_device(ptr, n, 0.1)
            _, mx, _ = r.grayscale_image(2.2)
            digits = max(1, (mx.bit_length() + 7) // 8)
            t_all = timed(lambda: cb.white_count_device(ptr, n, 0.1))
            t_p0 = timed(lambda: cb.white_count_device(ptr, n, 0.0))
            say(size=size, what="white_count_device p=0.1", max=mx, white=white, lit=lit, clipped=clipped, passes=1 + digits,
                bytes_per_pass=8 * n, **t_all)
            say(size=size, what="white_count_device p=0 (pass 0 only)", **t_p0,
                pass0_bytes_per_s=8 * n / t_p0["median_s"],
                digit_pass_bytes_per_s=8 * n * digits / max(t_all["median_s"] - t_p0["median_s"], 1e-9))
            r.set_white_clip(0.1)
            r.grayscale_image(2.2)
            say(size=size, what="grayscale_image clip 0.1", **timed(lambda: r.grayscale_image(2.2)))
            assert r.last_white() == (white, lit, clipped)
            r.set_white_clip(0)
            say(size=size, what="grayscale_image unclipped again", **timed(lambda: r.grayscale_image(2.2)))

if which == "current":  # the two README renders: what the image shows with and without the clip
    for name, m, setup in (("basilica", 2000, lambda r: (r.set_julia((-1.0, 0.0)), r.set_bounded())),
                           ("feigenbaum", 20000, lambda r: (r.set_projection([1, 0, 0, 0, 0, 0, 1, 0]), r.set_bounded()))):
        dims = cb.FractalDimensions.make(4096, 4096)
        with cb.Renderer(dims, cb.IterationControl(m, 20)) as r:
            setup(r)
            t0, done = time.perf_counter(), 0
            while time.perf_counter() - t0 < 12.0:
                r.render_passes(8)
                r.finish()
                done += 8
            plain, mx, scale = r.grayscale_image(1.0)
            levels_plain = int(np.unique(plain).size)
            below = int(np.count_nonzero(plain.astype(np.uint16) < 256))
            r.set_white_clip(0.1)
            clip, mx2, scale2 = r.grayscale_image(1.0)
            white, lit, clipped = r.last_white()
            hist = r.read_histogram()
            top = np.sort(hist.reshape(-1))[-5:].tolist()
            say(what="readme render", name=name, passes=done, seconds=time.perf_counter() - t0, max=mx, white=white, lit=lit,
                clipped=clipped, levels_unclipped=levels_plain, levels_clipped=int(np.unique(clip).size),
                lit_pixels_below_level_256_unclipped=below - (4096 * 4096 - lit),
                lit_pixels_below_level_256_clipped=int(np.count_nonzero(clip.astype(np.uint16) < 256)) - (4096 * 4096 - lit),
                median_lit=int(np.median(hist[hist > 0])), top5=top, scale_unclipped=scale, scale_clipped=scale2)
