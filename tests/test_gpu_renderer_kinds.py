"""What a renderer may become, as one table: every starting renderer against every setter.

The per-feature files (test_gpu_project.py .. test_gpu_phoenix.py) check the pairs that existed when each was written; this
one pins the whole table of cb_renderer_set_{focus, projection, julia, palette, depth, depth_palette, frames, phoenix}.  The
table below is literal data, copied from the behaviour of the library, and not computed from a restatement of its rule.

Each cell is tried on a fresh copy of its starting renderer, so that an accepted setter cannot mask the next.  A refusal is
hipErrorInvalidValue and leaves the renderer as it was: every getter, the histogram's shape and its contents.  An acceptance
gives the histogram the planes of the new kind, refuses the same setter a second time, and one pass then runs the kernel of
that kind and accounts for every increment.

Shapes, the smallest at which all of this can go wrong: a 16 x 16 canvas, -m 100 -c 20, 256 threads (a pass is 50 samples
per thread), a palette of 100 entries, 4 slices with a table of 4 entries, 2 frames.  A focus needs a probe that marks cells:
the 64 x 64 box of test_gpu_phoenix.py with -m 300 -c 20 and 4096 threads, for the focused starting renderer (whose valid
palette then has 300 entries) and for the one cell in which a plain renderer takes a focus.
"""

import ctypes as C

import numpy as np
import pytest

import plot_reference as plot
from plot_harness import INVALID

pytestmark = pytest.mark.gpu

SETTERS = ("focus", "projection", "julia", "palette", "depth", "depth_palette", "frames", "phoenix")
# 1: accepted, 0: refused; a column per setter, in the order of SETTERS
TABLE = {
    #                          focus proj julia pal depth dpal frames phoenix
    "plain":                     (1,   1,   1,   1,   0,    0,    0,    0),
    "channels":                  (0,   0,   0,   0,   0,    0,    0,    0),
    "focused":                   (0,   0,   0,   0,   0,    0,    0,    0),
    "projected":                 (0,   0,   0,   1,   1,    1,    1,    1),
    "julia":                     (0,   0,   0,   1,   1,    1,    1,    1),
    "plain + palette":           (0,   0,   0,   0,   0,    0,    0,    0),
    "projected + palette":       (0,   0,   0,   0,   0,    0,    0,    0),
    "julia + palette":           (0,   0,   0,   0,   0,    0,    0,    0),
    "projected + depth":         (0,   0,   0,   0,   0,    0,    0,    0),
    "julia + depth palette":     (0,   0,   0,   0,   0,    0,    0,    0),
    "projected + frames":        (0,   0,   0,   0,   0,    0,    0,    0),
    "julia + phoenix":           (0,   0,   0,   0,   0,    0,    0,    0),
    "plain after a pass":        (0,   0,   0,   0,   0,    0,    0,    0),
    "projected after a pass":    (0,   0,   0,   0,   0,    0,    0,    0),
}
# after an acceptance: the planes of the histogram and what cb_debug_last_draw_kernel() says after one pass
SLICES, FRAMES = 4, 2
PLANES = {"focus": 1, "projection": 1, "julia": 1, "palette": 3, "depth": SLICES, "depth_palette": 3, "frames": FRAMES,
          "phoenix": 1}
KERNEL = {"focus": 6, "projection": 8, "julia": 12, "palette": 14, "depth": 18, "depth_palette": 20, "frames": 22,
          "phoenix": 24}

# c and p of test_gpu_phoenix.py's Julia case: of a pass's 12 800 samples its restatement (phoenix_reference.py) plots 1115
# points with this c and 4546 with a sampled one; with p = (-0.5, 0) and this c it plots none
JULIA_C, PHOENIX_P, DEPTH = (-0.8, 0.156), (0.25, 0.0), ("cr", -2.0, 0.5, SLICES)


def make(cb, name, focus_inputs):
    """The starting renderer `name`; focus_inputs: on the canvas whose probe marks cells."""
    if focus_inputs:
        dims, it, threads = cb.FractalDimensions.make(64, 64, -0.2, 0.0, -0.9, -0.7), cb.IterationControl(300, 20), 4096
    else:
        dims, it, threads = cb.FractalDimensions.make(16, 16), cb.IterationControl(100, 20), 256
    if name == "channels":
        return cb.Renderer(dims, [(100, 20), (50, 5)], device=0, n_threads=threads)
    r = cb.Renderer(dims, it, device=0, n_threads=threads)
    first, _, rest = name.partition(" ")
    if first == "focused":
        r.set_focus(6, 4, 1)
    elif first == "projected":
        r.set_projection(cb.IDENTITY_PROJECTION)
    elif first == "julia":
        r.set_julia(JULIA_C)
    if rest == "+ palette":
        r.set_palette(plot.demo_table(100))
    elif rest == "+ depth":
        r.set_depth(DEPTH)
    elif rest == "+ depth palette":
        r.set_depth_palette(DEPTH, plot.demo_table(SLICES))
    elif rest == "+ frames":
        r.set_frames(np.array([cb.IDENTITY_PROJECTION] * FRAMES))
    elif rest == "+ phoenix":
        r.set_phoenix(PHOENIX_P)
    elif rest == "after a pass":
        r.render_passes(1)
    return r


def call(cb, r, setter):
    """The setter with valid arguments for this renderer -> the code it returned."""
    try:
        if setter == "focus":
            r.set_focus(6, 4, 1)
        elif setter == "projection":
            r.set_projection(cb.IDENTITY_PROJECTION)
        elif setter == "julia":
            r.set_julia(JULIA_C)
        elif setter == "palette":
            first = r.iterations if isinstance(r.iterations, cb.IterationControl) else cb.IterationControl(*r.iterations[0])
            r.set_palette(plot.demo_table(first.max_escape_iterations))  # (a channel renderer: of its first window)
        elif setter == "depth":
            r.set_depth(DEPTH)
        elif setter == "depth_palette":
            r.set_depth_palette(DEPTH, plot.demo_table(SLICES))
        elif setter == "frames":
            r.set_frames(np.array([cb.IDENTITY_PROJECTION] * FRAMES))
        elif setter == "phoenix":
            r.set_phoenix(PHOENIX_P)
    except cb.CudabrotError as e:
        return e.code
    return 0


def getters(r):
    """What every getter answers, comparable with ==."""
    projection, depth, depth_palette, frames = r.projection(), r.depth(), r.depth_palette(), r.frames()
    return (
        None if projection is None else projection.tolist(),
        r.julia(),
        r.palette(),
        None if depth is None else depth.as_tuple(),
        None if depth_palette is None else (depth_palette[0].as_tuple(), depth_palette[1]),
        None if frames is None else frames.tolist(),
        r.phoenix(),
        r.focus_cells(),
    )


def library_planes(cb, r):
    """The planes the library itself counts: cb_renderer_grayscale_plane takes 0 .. planes - 1 and refuses the next."""
    gray = np.empty((r.dims.h, r.dims.w), dtype=">u2")
    n = 0
    while cb.lib.cb_renderer_grayscale_plane(r._h, n, 1.0, 0, gray.ctypes.data, None, None) == 0:
        n += 1
        assert n <= 8
    return n


@pytest.mark.parametrize("name", list(TABLE))
def test_every_setter_on_a_fresh_copy_of_the_starting_renderer(cb, name):
    assert len(TABLE[name]) == len(SETTERS)
    for setter, accepted in zip(SETTERS, TABLE[name]):
        where = (name, setter)
        # a focus has to find cells: the focused starting renderer, and the plain one in the cell that takes a focus
        focus_inputs = name == "focused" or (setter == "focus" and accepted)
        with make(cb, name, focus_inputs) as r:
            h, w = r.dims.h, r.dims.w
            before, hist = getters(r), r.read_histogram()
            rendered = name.endswith("after a pass")
            assert (int(hist.sum()) > 0) == rendered, where
            code = call(cb, r, setter)
            if not accepted:
                assert code == INVALID, where
                assert getters(r) == before, where
                after = r.read_histogram()
                assert after.shape == hist.shape and np.array_equal(after, hist), where
                assert library_planes(cb, r) == (hist.shape[0] if hist.ndim == 3 else 1), where
                continue
            assert code == 0, where
            planes = PLANES[setter]
            assert r.read_histogram().shape == ((h, w) if planes == 1 else (planes, h, w)), where
            assert library_planes(cb, r) == planes, where
            assert call(cb, r, setter) == INVALID, where  # once
            r.render_passes(1)
            assert cb.lib.cb_debug_last_draw_kernel() == KERNEL[setter], where
            total = int(r.read_histogram().sum())
            assert total == r.read_counters().as_dict()["increments"] > 0, where


# The one assertion of this file that fails before the Renderer class asked the library for its planes: it kept counters of
# its own, which a setter called through cb.lib left stale -- read_histogram then handed the library a one-plane buffer for a
# histogram of several.  Everything above passes on either side of that change.
def test_python_renderer_follows_a_setter_called_through_the_library(cb):
    dims, it = cb.FractalDimensions.make(16, 16), cb.IterationControl(100, 20)
    identity = (C.c_double * 8)(*cb.IDENTITY_PROJECTION)
    depth = cb.Depth.make(*DEPTH)
    table = np.ascontiguousarray(plot.demo_table(100), dtype=np.uint32)
    slice_table = np.ascontiguousarray(plot.demo_table(SLICES), dtype=np.uint32)
    frames = np.ascontiguousarray([cb.IDENTITY_PROJECTION] * FRAMES, dtype=np.float64)
    cases = (
        (lambda r: cb.lib.cb_renderer_set_palette(r._h, table.ctypes.data, table.size), 3, "palette_image", (16, 16, 3)),
        (lambda r: cb.lib.cb_renderer_set_depth(r._h, C.byref(depth)), SLICES, "depth_image", (SLICES, 16, 16)),
        (lambda r: cb.lib.cb_renderer_set_depth_palette(r._h, C.byref(depth), slice_table.ctypes.data, SLICES), 3,
         "depth_palette_image", (16, 16, 3)),
        (lambda r: cb.lib.cb_renderer_set_frames(r._h, frames.ctypes.data, FRAMES), FRAMES, "frames_image", (FRAMES, 16, 16)),
    )
    for setter, planes, image, shape in cases:
        with cb.Renderer(dims, it, device=0, n_threads=256) as r:
            assert cb.lib.cb_renderer_set_projection(r._h, identity) == 0
            assert setter(r) == 0
            r.render_passes(1)
            hist = r.read_histogram()
            assert hist.shape == (planes, 16, 16), image
            assert int(hist.sum()) == r.read_counters().as_dict()["increments"] > 0, image
            assert getattr(r, image)()[0].shape == shape, image
            r.write_histogram(hist)  # (its size check counts the same planes)
            assert np.array_equal(r.read_histogram(), hist), image
