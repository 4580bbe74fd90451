#!/usr/bin/env python3
"""Times the equalised image on real renders, on a GPU (the record is profiles/equalize_rate.txt).

usage: equalize_rate.py run PARENT_PKGROOT OUT.txt WHERE [SIZE...]   the whole measurement: one child process per case
       equalize_rate.py child PKGROOT {current|parent} SIZE          one case, JSON lines on stdout

WHERE is the machine and the day as the record's first line is to name them, e.g. "one MI355X, 2026-10-21".

PARENT_PKGROOT is a directory that holds a built cudabrot_amd package of the commit before this one; its unflagged image
call is timed beside this tree's, the two alternating (current, parent, current, parent).  For every SIZE a SIZE x SIZE
canvas is rendered (1000 / 20 iterations, 64 passes up to 4096, 32 above) and, three repetitions each by the host clock
around calls that end in a device synchronise, medians with their ranges:
  cb_renderer_grayscale_image unflagged (both trees);
  this tree only: a device-to-device copy of the counters' bytes (torch, same process), cb_white_count_device at p = 0
  (one sweep), cb_equalize_bins_device (one sweep into 56 320 bins, with the window named in equalize.hip);
  cb_tone_map_device in its table form and cb_tone_map_device_equalized, whole calls -- each a sweep, a host table, an
  upload and the lookup kernel: the lookup kernels alone are not separated by a host clock;
  cb_renderer_grayscale_image equalised, and what it found."""
import json
import os
import re
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(f, reps=3):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts)}


def child(pkgroot, which, size):
    sys.path.insert(0, pkgroot)
    import cudabrot_amd as cb

    assert cb.library_path().startswith(pkgroot), cb.library_path()

    def say(**kw):
        print(json.dumps(dict(kw, which=which, size=size)), flush=True)

    n = size * size
    with cb.Renderer(cb.FractalDimensions.make(size, size), cb.IterationControl(1000, 20)) as r:
        r.render_passes(64 if size <= 4096 else 32)
        r.finish()
        r.grayscale_image(2.2)  # warm
        say(what="grayscale_image unflagged", **timed(lambda: r.grayscale_image(2.2)))
        if which != "current":
            return
        import torch

        ptr = r.device_histogram
        a = torch.zeros(n, dtype=torch.int64, device="cuda:0")
        b = torch.zeros(n, dtype=torch.int64, device="cuda:0")

        def copy():
            b.copy_(a)
            torch.cuda.synchronize()

        copy()
        say(what="device copy of 8n bytes (read + write)", bytes=8 * n, **timed(copy))
        del a, b
        cb.white_count_device(ptr, n, 0.0)
        t = timed(lambda: cb.white_count_device(ptr, n, 0.0))
        say(what="white_count_device p=0 (one sweep)", bytes_per_s=8 * n / t["median_s"], **t)
        bins, lit, mx = cb.equalize_bins_device(ptr, n)
        t = timed(lambda: cb.equalize_bins_device(ptr, n))
        say(what="equalize_bins_device (one sweep)", window=window(), lit=lit, max=mx, keys=int((bins > 0).sum()),
            keys_at_or_above_window=int((bins[window():] > 0).sum()), counters_at_or_above_window=int(bins[window():].sum()),
            bytes_per_s=8 * n / t["median_s"], **t)
        gray = torch.zeros(n, dtype=torch.int16, device="cuda:0")
        if mx < 1 << 24:
            cb.tone_map_device(ptr, size, size, 2.2, gray.data_ptr(), mode=cb.CB_TONE_LUT)
            say(what="tone_map_device, table form (whole call)",
                **timed(lambda: cb.tone_map_device(ptr, size, size, 2.2, gray.data_ptr(), mode=cb.CB_TONE_LUT)))
        cb.tone_map_device_equalized(ptr, size, size, 2.2, gray.data_ptr())
        say(what="tone_map_device_equalized (whole call)",
            **timed(lambda: cb.tone_map_device_equalized(ptr, size, size, 2.2, gray.data_ptr())))
        del gray
        r.set_equalize()
        r.grayscale_image(2.2)
        found = r.last_equalize()
        say(what="grayscale_image equalised", lit=found[0], keys=found[1], levels=found[2],
            **timed(lambda: r.grayscale_image(2.2)))
        r.set_equalize(False)
        say(what="grayscale_image unflagged again", **timed(lambda: r.grayscale_image(2.2)))


def window():
    with open(os.path.join(HERE, "cudabrot_amd", "csrc", "equalize.hip")) as f:
        return int(re.search(r"kWindow = (\d+);", f.read()).group(1))


def header(where, sizes):
    """The first lines of the record: where and when, the sizes, and the window equalize.hip names."""
    return ("# tools/equalize_rate.py on %s, sizes %s, window W = %d (DESIGN.md 4.26):\n"
            "# this tree (`current`) and the commit before it (`parent`), one child process per case, alternating; three\n"
            "# repetitions per figure, seconds by the host clock around calls that end in a device synchronise.  The image\n"
            "# calls include the copy of the 16-bit image to pageable host memory.\n"
            % (where, " and ".join(str(s) for s in sizes), window()))


def run(parent_root, out_path, where, sizes):
    with open(out_path, "w") as out:
        out.write(header(where, sizes))
        for size in sizes:
            for which, root in (("current", HERE), ("parent", parent_root)) * 2:
                done = subprocess.run([sys.executable, os.path.abspath(__file__), "child", root, which, str(size)],
                                      stdout=subprocess.PIPE, text=True, timeout=900)
                out.write(done.stdout)
                out.flush()
                print(done.stdout, end="", flush=True)
                if done.returncode != 0:  # nothing more is started on a device that a case has failed on
                    out.write("# %s at %d ended with status %d: stopped here\n" % (which, size, done.returncode))
                    return done.returncode
    return 0


if __name__ == "__main__":
    if sys.argv[1] == "child":
        child(sys.argv[2], sys.argv[3], int(sys.argv[4]))
    else:
        sys.exit(run(os.path.abspath(sys.argv[2]), sys.argv[3], sys.argv[4], [int(s) for s in sys.argv[5:]]))
