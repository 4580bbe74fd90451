#!/usr/bin/env python3
"""Times the output stage on real renders, on a GPU -- the tone map, --white-clip, --equalize, --density-filter (DESIGN.md
4.24-4.26): one tool, one method, one record (profiles/output_rate.txt).

usage: output_rate.py run PARENT_PKGROOT OUT.txt WHERE [SIZE...]   the whole measurement: one child process per case
       output_rate.py child PKGROOT {current|parent} SIZE          one case, JSON lines on stdout
       output_rate.py --list [SIZE...]                             the rows and the children `run` would start
       output_rate.py local PKGROOT OUT.txt WHERE SIZE...          --local-equalize against --equalize
       output_rate.py local-child PKGROOT SIZE                     one size of it, JSON lines on stdout
       output_rate.py local-trace TRACE.csv                        kernel medians of a local-child run under a kernel trace
       output_rate.py local-clip PKGROOT                           what --local-equalize's clip does to one render
       output_rate.py picture PKGROOT [SECONDS [PASSES]]           what the density filter does to a short render
       output_rate.py readme PKGROOT                               README.md's two --bounded renders, clipped and not

WHERE is the machine and the day as the record's first line is to name them, e.g. "one MI355X, 2026-10-21".  PKGROOT is a
directory that holds a built cudabrot_amd package; PARENT_PKGROOT one of the commit before this one.  Neither the C ABI nor
the Python API differs between the two, so every row is timed in BOTH trees, the two alternating (current, parent, current,
parent), each case in a process of its own under its own time limit.  The first child that fails or runs out of time ends
the run: nothing more is started on the device after it.  --list touches neither the library nor a device.

A case: a SIZE x SIZE canvas is rendered (1000 / 20 iterations, 64 passes up to 4096, 32 above) and every row of ROWS is
called once to warm it and then three times, seconds by the host clock around calls that end in a device synchronise.  The
image calls include the copy of the 16-bit image to pageable host memory; the device calls are whole calls -- a sweep, a
host table, an upload and the lookup kernel: the lookup kernels alone are not separated by a host clock.

The record closes with one line per row and size: the branch's median over its six repetitions against the parent's
largest repetition plus the parent's own spread (largest minus smallest) that day; a row within that is `unchanged`.

local: the same render per SIZE, one child process per size under its own time limit, the first that fails ends the run.
In ONE process the two global calls -- equalize_bins_device, tone_map_device_equalized -- and, for 1 x 1, 8 x 8 and 16 x 16
tiles at the binary's default clip, local_equalize_bins_device and tone_map_device_local_equalized are each called once to
warm them and then three times; the record (profiles/local_equalize_rate.txt) gives the median and the range of each, and
closes with the local calls as ratios to the global ones.  The bins entry point expands every tile's bins to all 56 320
keys on the host, which the image call does not; the kernels alone are not separated by a host clock.

local-trace: TRACE.csv is the kernel trace a profiler wrote of one `local-child` run (rocprofv3 --kernel-trace
--output-format csv -- python3 tools/output_rate.py local-child PKGROOT SIZE; profiles/local_equalize_SIZE_kernel_trace.csv
are two).  Prints the median and the range, in microseconds, of every dispatch of the output stage's kernels, the two local
kernels grid by grid: a child dispatches local_bins_kernel nine times and local_map_kernel five times per grid before the
renderer's image calls, in LOCAL_GRIDS' order.

local-clip: a 2048 x 2048 render (1000 / 20 iterations, 64 passes), its image unflagged, equalised and locally equalised in
8 x 8 tiles at clips 2, 4, 8 and off (device bytes and numbers checked against the host function's): per tile with 1000 lit
pixels or more, the span between the 5th and the 95th percentile of the lit pixels' output values and the number of
distinct values (profiles/local_equalize_clip.txt).

picture: a 4096 x 4096 default render (100 / 20 iterations) of SECONDS seconds (default 3), its image without and with
--density-filter 4, 4:0.5:4 and 8, against a run of 64 times as many passes on other generators: the RMS difference of the
16-bit images (gamma 1, each normalised to its own maximum, and again scaled to one mean level), the pixels that are 0 in
the short image and lit in the long one, and the RMS difference in counts between the (filtered) counters and the long run's
counters / 64, over all pixels and over the pixels where fewer than 4, 4 to 16 and 16 or more counts are expected.  With
PASSES (a multiple of 8) the short run is that many passes instead of SECONDS seconds: a sparse histogram.

readme: README.md's two --bounded renders at 4096 x 4096 for about 12 s each, and what their images hold with and without
--white-clip 0.1."""
import json
import os
import re
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS, LIMIT = 3, 900.0
GAMMA, CLIP, RADII = 2.2, 0.1, (4, 8)
# The rows of a case, in the order they run: the renderer's image call as each flag sets it, the device calls under them,
# and the device-to-device copy of the counters' bytes as the yardstick.
ROWS = (["grayscale_image unflagged", "device copy of 8n bytes (read + write)", "white_count_device p=0 (one sweep)",
         "white_count_device p=%g" % CLIP, "equalize_bins_device (one sweep)", "tone_map_device, table form (whole call)",
         "tone_map_device_equalized (whole call)"]
        + ["density_filter_device R=%d (with its maximum pass)" % r for r in RADII]
        + ["grayscale_image --white-clip %g" % CLIP, "grayscale_image equalised"]
        + ["grayscale_image --density-filter %d" % r for r in RADII] + ["grayscale_image unflagged again"])


def passes(size):
    return 64 if size <= 4096 else 32


def timed(f, reps=REPS):
    """f() once to warm it, then `reps` times by the host clock."""
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "reps_s": ts}


def load(pkgroot):
    sys.path.insert(0, pkgroot)
    import cudabrot_amd as cb

    assert cb.library_path().startswith(pkgroot), cb.library_path()
    return cb


def rendered(cb, size, max_iter=1000, **kw):
    """The one render set-up: a size x size canvas at max_iter / 20 iterations."""
    return cb.Renderer(cb.FractalDimensions.make(size, size), cb.IterationControl(max_iter, 20), **kw)


def child(pkgroot, which, size):
    cb = load(pkgroot)
    import torch

    def say(what, t, **kw):
        assert what == ROWS[say.at], (what, ROWS[say.at])  # the rows --list names, in their order
        say.at += 1
        print(json.dumps(dict(kw, what=what, which=which, size=size, **t)), flush=True)

    say.at = 0
    n = size * size
    with rendered(cb, size) as r:
        r.render_passes(passes(size))
        r.finish()
        image = lambda: r.grayscale_image(GAMMA)  # noqa: E731
        say("grayscale_image unflagged", timed(image))
        ptr, stream = r.device_histogram, torch.cuda.current_stream().cuda_stream
        a = torch.zeros(n, dtype=torch.int64, device="cuda:0")
        b = torch.zeros(n, dtype=torch.int64, device="cuda:0")  # the density filter's output too

        def copy():
            b.copy_(a)
            torch.cuda.synchronize()

        t_copy = timed(copy)
        say("device copy of 8n bytes (read + write)", t_copy, bytes=8 * n, bytes_per_s=2 * 8 * n / t_copy["median_s"])
        del a
        t_p0 = timed(lambda: cb.white_count_device(ptr, n, 0.0))
        say("white_count_device p=0 (one sweep)", t_p0, bytes_per_s=8 * n / t_p0["median_s"])
        white, lit, clipped = cb.white_count_device(ptr, n, CLIP)
        mx = image()[1]
        digits = max(1, (mx.bit_length() + 7) // 8)
        t = timed(lambda: cb.white_count_device(ptr, n, CLIP))
        say("white_count_device p=%g" % CLIP, t, max=mx, white=white, lit=lit, clipped=clipped, passes=1 + digits,
            bytes_per_pass=8 * n, digit_pass_bytes_per_s=8 * n * digits / max(t["median_s"] - t_p0["median_s"], 1e-9))
        bins, lit_bins, mx = cb.equalize_bins_device(ptr, n)
        t = timed(lambda: cb.equalize_bins_device(ptr, n))
        say("equalize_bins_device (one sweep)", t, window=window(), lit=lit_bins, max=mx, keys=int((bins > 0).sum()),
            keys_at_or_above_window=int((bins[window():] > 0).sum()), counters_at_or_above_window=int(bins[window():].sum()),
            bytes_per_s=8 * n / t["median_s"])
        gray = torch.zeros(n, dtype=torch.int16, device="cuda:0")
        assert mx < 1 << 24, mx  # the table form
        say("tone_map_device, table form (whole call)",
            timed(lambda: cb.tone_map_device(ptr, size, size, GAMMA, gray.data_ptr(), mode=cb.CB_TONE_LUT)))
        say("tone_map_device_equalized (whole call)",
            timed(lambda: cb.tone_map_device_equalized(ptr, size, size, GAMMA, gray.data_ptr())))
        del gray
        for radius in RADII:
            table = cb.density_thresholds(radius, 0.5, 1)
            t = timed(lambda: cb.density_filter_device(ptr, size, size, 1, 1, table, b.data_ptr(), stream=stream))
            say("density_filter_device R=%d (with its maximum pass)" % radius, t, thresholds=table[1:],
                bytes_per_s=2 * 8 * n / t["median_s"], times_the_copy=t["median_s"] / t_copy["median_s"])
        del b
        r.set_white_clip(CLIP)
        t = timed(image)
        assert r.last_white() == (white, lit, clipped)
        say("grayscale_image --white-clip %g" % CLIP, t)
        r.set_white_clip(0)
        r.set_equalize()
        t = timed(image)
        found = r.last_equalize()
        say("grayscale_image equalised", t, lit=found[0], keys=found[1], levels=found[2])
        r.set_equalize(False)
        for radius in RADII:
            r.set_density_filter(radius)
            say("grayscale_image --density-filter %d" % radius, timed(image))
            r.set_density_filter(0)
        say("grayscale_image unflagged again", timed(image))
    assert say.at == len(ROWS)


def window():
    with open(os.path.join(HERE, "cudabrot_amd", "csrc", "equalize.hip")) as f:
        return int(re.search(r"kWindow = (\d+);", f.read()).group(1))


def header(where, sizes):
    """The first lines of the record: where and when, the sizes, and the window equalize.hip names."""
    return ("# tools/output_rate.py on %s, sizes %s, window W = %d (DESIGN.md 4.24-4.26):\n"
            "# this tree (`current`) and the commit before it (`parent`), every row in both, one child process per case,\n"
            "# alternating; three repetitions per figure after one call to warm it, seconds by the host clock around calls\n"
            "# that end in a device synchronise.  The image calls include the copy of the 16-bit image to pageable host memory.\n"
            % (where, " and ".join(str(s) for s in sizes), window()))


def child_command(root, which, size):
    return [sys.executable, os.path.abspath(__file__), "child", root, which, str(size)]


def children(parent_root, sizes):
    """(which, root, size) of every child, in the order `run` starts them."""
    return [(which, root, size) for size in sizes for which, root in (("current", HERE), ("parent", parent_root)) * 2]


def verdicts(lines):
    """One line per (row, size) of the JSON lines both trees wrote: the branch's median over all its repetitions against the
    parent's largest repetition plus the parent's spread."""
    reps = {}
    for line in lines:
        rec = json.loads(line)
        reps.setdefault((rec["size"], rec["what"]), {}).setdefault(rec["which"], []).extend(rec["reps_s"])
    out = []
    for (size, what), by in reps.items():
        if "current" in by and "parent" in by:
            median, lo, hi = statistics.median(by["current"]), min(by["parent"]), max(by["parent"])
            out.append("# %5d  %-50s current median %.6g s; parent %.6g .. %.6g s, spread %.6g s: %s\n"
                       % (size, what, median, lo, hi, hi - lo, "unchanged" if median <= hi + (hi - lo) else "OUTSIDE the margin"))
    return out


def run(parent_root, out_path, where, sizes, command=child_command, limit=LIMIT):
    lines = []
    with open(out_path, "w") as out:
        out.write(header(where, sizes))
        for which, root, size in children(parent_root, sizes):
            try:
                done = subprocess.run(command(root, which, size), stdout=subprocess.PIPE, text=True, timeout=limit)
                text, status = done.stdout, done.returncode
            except subprocess.TimeoutExpired as e:
                text, status = (e.stdout.decode() if isinstance(e.stdout, bytes) else e.stdout or ""), 124
            out.write(text)
            out.flush()
            print(text, end="", flush=True)
            if status != 0:  # nothing more is started on a device that a case has failed on
                out.write("# %s at %d ended with status %d: stopped here\n" % (which, size, status))
                return status if status > 0 else 128 - status
            lines += text.splitlines()
        out.write("# row by row: the branch's median of six repetitions, the parent's six, and whether the median is within\n"
                  "# the parent's largest plus the parent's spread\n")
        out.writelines(verdicts(lines))
    return 0


LOCAL_GRIDS, LOCAL_CLIP_Q = (1, 8, 16), 1024


def local_child(pkgroot, size):
    cb = load(pkgroot)
    import torch

    def row(what, t, **kw):
        print(json.dumps(dict(kw, what=what, size=size, **t)), flush=True)

    n = size * size
    with rendered(cb, size) as r:
        r.render_passes(passes(size))
        r.finish()
        ptr = r.device_histogram
        gray = torch.zeros(n, dtype=torch.int16, device="cuda:0")
        bins, lit, mx = cb.equalize_bins_device(ptr, n)
        row("equalize_bins_device (one sweep)", timed(lambda: cb.equalize_bins_device(ptr, n)), lit=lit, max=mx,
            keys=int((bins > 0).sum()), keys_per_tile_array=cb.equalize_key(mx) + 1)
        row("tone_map_device_equalized (whole call)",
            timed(lambda: cb.tone_map_device_equalized(ptr, size, size, GAMMA, gray.data_ptr())))
        for tiles in LOCAL_GRIDS:
            row("local_equalize_bins_device %dx%d (maximum, sweep, 56320 keys a tile to the caller)" % (tiles, tiles),
                timed(lambda: cb.local_equalize_bins_device(ptr, size, size, 1, tiles, tiles)), tiles=tiles)
            found = cb.tone_map_device_local_equalized(ptr, size, size, 1, tiles, tiles, LOCAL_CLIP_Q, GAMMA, gray.data_ptr())
            row("tone_map_device_local_equalized %dx%d clip %d/256 (whole call)" % (tiles, tiles, LOCAL_CLIP_Q),
                timed(lambda: cb.tone_map_device_local_equalized(ptr, size, size, 1, tiles, tiles, LOCAL_CLIP_Q, GAMMA,
                                                                 gray.data_ptr())),
                tiles=tiles, lit=found[2], lit_tiles=found[3], moved=found[4])
        r.set_equalize()
        row("grayscale_image equalised", timed(lambda: r.grayscale_image(GAMMA)))
        r.set_equalize(False)
        for tiles in LOCAL_GRIDS:
            r.set_local_equalize(tiles)
            row("grayscale_image locally equalised %dx%d" % (tiles, tiles), timed(lambda: r.grayscale_image(GAMMA)), tiles=tiles)
        r.set_local_equalize(0)


def local_ratios(lines):
    """The local calls as ratios of medians to the global ones, one line per size and grid."""
    by = {}
    for line in lines:
        rec = json.loads(line)
        by[(rec["size"], rec["what"].split(" ")[0], rec.get("tiles", 0))] = rec
    out = []
    for (size, what, tiles), rec in by.items():
        if what == "tone_map_device_local_equalized":
            sweep, call = by[(size, "equalize_bins_device", 0)], by[(size, "tone_map_device_equalized", 0)]
            out.append("# %5d  %2dx%-2d tiles: bins call %.6g s = %.2f of the global one; whole call %.6g s (%.6g .. %.6g) = %.2f of "
                       "the global one\n"
                       % (size, tiles, tiles, by[(size, "local_equalize_bins_device", tiles)]["median_s"],
                          by[(size, "local_equalize_bins_device", tiles)]["median_s"] / sweep["median_s"], rec["median_s"],
                          rec["min_s"], rec["max_s"], rec["median_s"] / call["median_s"]))
    return out


def local(pkgroot, out_path, where, sizes, limit=LIMIT):
    lines = []
    with open(out_path, "w") as out:
        out.write("# tools/output_rate.py local on %s, sizes %s (DESIGN.md 4.28): the global and the tile-wise calls in one\n"
                  "# process per size; three repetitions per figure after one call to warm it, seconds by the host clock around\n"
                  "# calls that end in a device synchronise\n" % (where, " and ".join(str(s) for s in sizes)))
        for size in sizes:
            command = [sys.executable, os.path.abspath(__file__), "local-child", pkgroot, str(size)]
            try:
                done = subprocess.run(command, stdout=subprocess.PIPE, text=True, timeout=limit)
                text, status = done.stdout, done.returncode
            except subprocess.TimeoutExpired as e:
                text, status = (e.stdout.decode() if isinstance(e.stdout, bytes) else e.stdout or ""), 124
            out.write(text)
            out.flush()
            print(text, end="", flush=True)
            if status != 0:  # nothing more is started on a device that a case has failed on
                out.write("# size %d ended with status %d: stopped here\n" % (size, status))
                return status if status > 0 else 128 - status
            lines += text.splitlines()
        out.write("# medians as ratios to the global calls of the same process\n")
        out.writelines(local_ratios(lines))
    return 0


def local_trace(path):
    import csv

    names = ("local_bins_kernel", "local_map_kernel", "equalize_bins_kernel", "equalize_map_kernel", "hist_max_kernel")
    took = {name: [] for name in names}
    with open(path) as f:
        for rec in csv.DictReader(f):
            for name in names:
                if name + "(" in rec["Kernel_Name"]:
                    took[name].append((int(rec["End_Timestamp"]) - int(rec["Start_Timestamp"])) / 1e3)

    def row(what, us):
        print(json.dumps({"what": what, "dispatches": len(us), "median_us": statistics.median(us), "min_us": min(us),
                          "max_us": max(us)}))

    for name in names[2:]:
        row(name, took[name])
    for at, tiles in enumerate(LOCAL_GRIDS):  # the device calls come before the renderer's: 9 and 5 dispatches a grid
        row("local_bins_kernel %dx%d" % (tiles, tiles), took["local_bins_kernel"][9 * at:9 * at + 9])
        row("local_map_kernel %dx%d" % (tiles, tiles), took["local_map_kernel"][5 * at:5 * at + 5])


def local_clip(pkgroot, size=2048, tiles=8):
    cb = load(pkgroot)
    import numpy as np

    with rendered(cb, size) as r:
        r.render_passes(64)
        r.finish()
        hist = r.read_histogram()
        images, found = {"unflagged": r.grayscale_image(GAMMA)[0].astype(np.uint16)}, {}
        r.set_equalize()
        images["--equalize"] = r.grayscale_image(GAMMA)[0].astype(np.uint16)
        r.set_equalize(False)
        for clip in (2, 4, 8, 0):
            name = "--local-equalize %d:%d" % (tiles, clip)
            r.set_local_equalize(tiles, tiles, 256 * clip)
            images[name] = r.grayscale_image(GAMMA)[0].astype(np.uint16)
            found[name] = r.last_local_equalize()
            host = cb.set_grayscale_pixels_local_equalized(hist, tiles, tiles, 256 * clip, GAMMA)
            assert np.array_equal(host[0], images[name]) and tuple(host[3:]) == found[name]
        r.set_local_equalize(0)
    lit, step = hist > 0, size // tiles
    print(json.dumps({"what": "local-clip: the render", "size": size, "tiles": [tiles, tiles], "gamma": GAMMA,
                      "max": int(hist.max()), "lit": int(lit.sum())}))
    for name, im in images.items():
        levels, spans = [], []
        for j in range(tiles):
            for i in range(tiles):
                where = (slice(j * step, (j + 1) * step), slice(i * step, (i + 1) * step))
                if lit[where].sum() >= 1000:
                    values = im[where][lit[where]]
                    levels.append(int(np.unique(values).size))
                    spans.append(float(np.subtract(*np.percentile(values, [95, 5]))))
        numbers = found.get(name)
        print(json.dumps({"what": "local-clip", "image": name, "tiles_counted": len(spans),
                          "span_5_to_95_percent_median": float(np.median(spans)), "span_5_to_95_percent_min": min(spans),
                          "distinct_values_median": float(np.median(levels)), "distinct_values_min": min(levels),
                          "lit_tiles": numbers[1] if numbers else None, "moved": numbers[2] if numbers else None}), flush=True)


def say(**kw):
    print(json.dumps(dict(kw, which="current")), flush=True)


def readme(pkgroot):
    cb = load(pkgroot)
    import numpy as np

    for name, m, setup in (("basilica", 2000, lambda r: (r.set_julia((-1.0, 0.0)), r.set_bounded())),
                           ("feigenbaum", 20000, lambda r: (r.set_projection([1, 0, 0, 0, 0, 0, 1, 0]), r.set_bounded()))):
        with rendered(cb, 4096, m) as r:
            setup(r)
            t0, done = time.perf_counter(), 0
            while time.perf_counter() - t0 < 12.0:
                r.render_passes(8)
                r.finish()
                done += 8
            plain, mx, scale = r.grayscale_image(1.0)
            levels_plain = int(np.unique(plain).size)
            below = int(np.count_nonzero(plain.astype(np.uint16) < 256))
            r.set_white_clip(CLIP)
            clip, mx2, scale2 = r.grayscale_image(1.0)
            white, lit, clipped = r.last_white()
            hist = r.read_histogram()
            top = np.sort(hist.reshape(-1))[-5:].tolist()
            say(what="readme render", name=name, passes=done, seconds=time.perf_counter() - t0, max=mx, white=white, lit=lit,
                clipped=clipped, levels_unclipped=levels_plain, levels_clipped=int(np.unique(clip).size),
                lit_pixels_below_level_256_unclipped=below - (4096 * 4096 - lit),
                lit_pixels_below_level_256_clipped=int(np.count_nonzero(clip.astype(np.uint16) < 256)) - (4096 * 4096 - lit),
                median_lit=int(np.median(hist[hist > 0])), top5=top, scale_unclipped=scale, scale_clipped=scale2)


def picture(pkgroot, seconds=3.0, short=0):
    cb = load(pkgroot)
    import numpy as np
    import torch

    size = 4096
    with rendered(cb, size, 100, seed=7) as r:  # the first launch allocates and loads: not timed
        r.render_passes(1)
        r.read_counters()
    with rendered(cb, size, 100) as r:
        t0, short_passes = time.perf_counter(), 0
        while (short_passes < short) if short else (time.perf_counter() - t0 < seconds):
            r.render_passes(8)
            r.read_counters()  # (waits for the device)
            short_passes += 8
        short_seconds = time.perf_counter() - t0
        counters = r.read_histogram()
        images = {"plain": r.grayscale_image(1.0)[0].astype(np.float64)}
        counts = {"plain": counters.astype(np.float64)}
        d_out = torch.empty(size * size, dtype=torch.int64, device="cuda:0")
        for name, params in (("4", (4, 0.5, 1)), ("4:0.5:4", (4, 0.5, 4)), ("8", (8, 0.5, 1))):
            r.set_density_filter(*params)
            images[name] = r.grayscale_image(1.0)[0].astype(np.float64)
            cb.density_filter_device(r.device_histogram, size, size, 1, 1, cb.density_thresholds(*params), d_out.data_ptr())
            counts[name] = d_out.cpu().numpy().view(np.uint64).reshape(size, size).astype(np.float64) / 256.0
    with rendered(cb, size, 100, seed=4242) as r:  # other generators: not the short run continued
        t0 = time.perf_counter()
        r.render_passes(64 * short_passes)
        r.read_counters()
        long_seconds = time.perf_counter() - t0
        truth = r.grayscale_image(1.0)[0].astype(np.float64)
        expected = r.read_histogram().astype(np.float64) / 64.0  # the counts the short run estimates
    lit = truth > 0
    say(what="picture: the two runs", size=size, short_passes=short_passes, short_seconds=short_seconds,
        long_passes=64 * short_passes, long_seconds=long_seconds, lit_pixels_short=int(np.count_nonzero(counters)),
        lit_pixels_long=int(np.count_nonzero(lit)), max_short=int(counters.max()), mean_count_short=float(counters.mean()),
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


def main(argv):
    what, rest = (argv[0], argv[1:]) if argv else ("", [])
    if what == "child" and len(rest) == 3:
        child(rest[0], rest[1], int(rest[2]))
    elif what == "run" and len(rest) >= 3:
        return run(os.path.abspath(rest[0]), rest[1], rest[2], [int(s) for s in rest[3:]])
    elif what == "--list":
        sizes = [int(s) for s in rest]
        print(header("WHERE", sizes), end="")
        for row in ROWS:
            print(json.dumps({"what": row}))
        for which, root, size in children("PARENT_PKGROOT", sizes):
            print(json.dumps({"child": which, "size": size, "passes": passes(size), "limit_s": LIMIT}))
    elif what == "local" and len(rest) >= 4:
        return local(os.path.abspath(rest[0]), rest[1], rest[2], [int(s) for s in rest[3:]])
    elif what == "local-child" and len(rest) == 2:
        local_child(os.path.abspath(rest[0]), int(rest[1]))
    elif what == "local-trace" and len(rest) == 1:
        local_trace(rest[0])
    elif what == "local-clip" and len(rest) == 1:
        local_clip(os.path.abspath(rest[0]))
    elif what == "picture" and 1 <= len(rest) <= 3:
        picture(os.path.abspath(rest[0]), float(rest[1]) if len(rest) > 1 else 3.0, int(rest[2]) if len(rest) > 2 else 0)
    elif what == "readme" and len(rest) == 1:
        readme(os.path.abspath(rest[0]))
    else:
        sys.exit(__doc__)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
