#!/usr/bin/env python3
"""Times the density filter on real renders, on a GPU (the record is profiles/density_rate.txt).

usage: density_rate.py PKGROOT {current|parent} OUT.jsonl rate SIZE...
       density_rate.py PKGROOT current OUT.jsonl picture [SECONDS [PASSES]]

PKGROOT is the directory that holds the cudabrot_amd package to load: this tree, or a build of the commit before it to time
its image call beside this one's (`parent`: only that call is timed).  One child process per case, run alternately.

rate: for every SIZE a SIZE x SIZE canvas is rendered (1000 / 20 iterations, 64 passes up to 4096, 32 above) and, medians of
three repetitions by the host clock around calls that end in a device synchronise: cb_renderer_grayscale_image without the
flag; then (`current`) cb_density_filter_device on the render's counters at R = 4 and R = 8 (alpha 0.5, n0 1), a
device-to-device copy of the same bytes in the same process as the yardstick (torch's copy of a contiguous tensor, 16 bytes
per lane), and the image call with the filter set.

picture: a 4096 x 4096 default render (100 / 20 iterations) of SECONDS seconds (default 3), its image without and with
--density-filter 4, 4:0.5:4 and 8, against a run of 64 times as many passes on other generators: the RMS difference of the
16-bit images (gamma 1, each normalised to its own maximum, and again scaled to one mean level), the pixels that are 0 in
the short image and lit in the long one, and the RMS difference in counts between the (filtered) counters and the long run's
counters / 64, over all pixels and over the pixels where fewer than 4, 4 to 16 and 16 or more counts are expected.  With
PASSES (a multiple of 8) the short run is that many passes instead of SECONDS seconds: a sparse histogram.

One JSON line per figure, appended to OUT.jsonl."""
import json
import statistics
import sys
import time

pkgroot, which, out_path, what = sys.argv[1:5]
rest = sys.argv[5:]
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


def rate(size):
    dims = cb.FractalDimensions.make(size, size)
    passes = 64 if size <= 4096 else 32
    with cb.Renderer(dims, cb.IterationControl(1000, 20)) as r:
        r.render_passes(passes)
        r.finish()
        n = size * size
        r.grayscale_image(2.2)  # warm
        say(size=size, what="grayscale_image without the flag", **timed(lambda: r.grayscale_image(2.2)))
        if which != "current":
            return
        import torch

        d_out = torch.empty(n, dtype=torch.int64, device="cuda:0")
        d_in = torch.empty(n, dtype=torch.int64, device="cuda:0")
        stream = torch.cuda.current_stream().cuda_stream

        def copy():
            d_in.copy_(d_out)
            torch.cuda.synchronize()

        copy()
        t_copy = timed(copy)
        say(size=size, what="device-to-device copy of the same bytes", bytes=8 * n, **t_copy,
            bytes_per_s=2 * 8 * n / t_copy["median_s"])
        hist = r.device_histogram
        for radius in (4, 8):
            table = cb.density_thresholds(radius, 0.5, 1)
            run = lambda: cb.density_filter_device(hist, size, size, 1, 1, table, d_out.data_ptr(), stream=stream)  # noqa: E731
            run()
            t = timed(run)
            say(size=size, what="density_filter_device R=%d (with its maximum pass)" % radius, thresholds=table[1:], **t,
                bytes_per_s=2 * 8 * n / t["median_s"], times_the_copy=t["median_s"] / t_copy["median_s"])
            r.set_density_filter(radius)
            r.grayscale_image(2.2)
            say(size=size, what="grayscale_image with --density-filter %d" % radius, **timed(lambda: r.grayscale_image(2.2)))
            r.set_density_filter(0)
        say(size=size, what="grayscale_image without the flag again", **timed(lambda: r.grayscale_image(2.2)))


def picture(seconds, passes):
    size = 4096
    dims = cb.FractalDimensions.make(size, size)
    import torch

    with cb.Renderer(dims, cb.IterationControl(100, 20), seed=7) as r:  # the first launch allocates and loads: not timed
        r.render_passes(1)
        r.read_counters()
    with cb.Renderer(dims, cb.IterationControl(100, 20)) as r:
        t0, short_passes = time.perf_counter(), 0
        while (short_passes < passes) if passes else (time.perf_counter() - t0 < seconds):
            r.render_passes(8)
            r.read_counters()  # (waits for the device)
            short_passes += 8
        short_seconds = time.perf_counter() - t0
        short = r.read_histogram()
        images = {"plain": r.grayscale_image(1.0)[0].astype(np.float64)}
        counts = {"plain": short.astype(np.float64)}
        d_out = torch.empty(size * size, dtype=torch.int64, device="cuda:0")
        for name, params in (("4", (4, 0.5, 1)), ("4:0.5:4", (4, 0.5, 4)), ("8", (8, 0.5, 1))):
            r.set_density_filter(*params)
            images[name] = r.grayscale_image(1.0)[0].astype(np.float64)
            cb.density_filter_device(r.device_histogram, size, size, 1, 1, cb.density_thresholds(*params), d_out.data_ptr())
            counts[name] = d_out.cpu().numpy().view(np.uint64).reshape(size, size).astype(np.float64) / 256.0
    with cb.Renderer(dims, cb.IterationControl(100, 20), seed=4242) as r:  # other generators: not the short run continued
        t0 = time.perf_counter()
        r.render_passes(64 * short_passes)
        r.read_counters()
        long_seconds = time.perf_counter() - t0
        truth = r.grayscale_image(1.0)[0].astype(np.float64)
        expected = r.read_histogram().astype(np.float64) / 64.0  # the counts the short run estimates
    lit = truth > 0
    say(what="picture: the two runs", size=size, short_passes=short_passes, short_seconds=short_seconds,
        long_passes=64 * short_passes, long_seconds=long_seconds, lit_pixels_short=int(np.count_nonzero(short)),
        lit_pixels_long=int(np.count_nonzero(lit)), max_short=int(short.max()), mean_count_short=float(short.mean()),
        pixels_expecting_below_4=int(np.count_nonzero(expected < 4)), pixels_expecting_16_or_more=int(np.count_nonzero(expected >= 16)))
    rms = lambda d: float(np.sqrt(np.mean(d ** 2))) if d.size else 0.0  # noqa: E731
    for name in images:
        im, c = images[name], counts[name]
        say(what="picture", density_filter=name,
            rms_of_normalised_16_bit_images=rms(im - truth),
            rms_of_images_scaled_to_one_mean=rms(im * (truth.mean() / im.mean()) - truth),
            zero_in_short_lit_in_long=int(np.count_nonzero((im == 0) & lit)),
            rms_counts=rms(c - expected), rms_counts_where_below_4_expected=rms((c - expected)[expected < 4]),
            rms_counts_where_4_to_16_expected=rms((c - expected)[(expected >= 4) & (expected < 16)]),
            rms_counts_where_16_or_more_expected=rms((c - expected)[expected >= 16]))


if what == "rate":
    for s in rest:
        rate(int(s))
elif what == "picture":
    picture(float(rest[0]) if rest else 3.0, int(rest[1]) if len(rest) > 1 else 0)
else:
    sys.exit(__doc__)
