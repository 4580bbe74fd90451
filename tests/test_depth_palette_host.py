"""The depth-palette render without a GPU (include/cudabrot_amd.h, "Depth-palette render"): the table-by-slice sink of the
CPU restatement (tests/plot_reference.c) against its depth sink without a table -- the definition's three consequences --
and against the definition by hand, the header's text, the stops' table, and the validation that needs no device."""

import ctypes as C
import math
import os

import numpy as np
import pytest

import plot_reference as plot
from plot_harness import INVALID, ref  # noqa: F401  (a fixture)

W, H, MAX, MIN, THREADS, LAUNCHES = 64, 48, 200, 2, 64, [20, 3]


def gradient(cb, n, stops):
    return cb.palette_from_stops(stops, n)


# ---- 1. the three consequences, against the depth sink ------------------------------------------------------------------

CASES = {
    "mandelbrot_cr_5": dict(d=("cr", -2.0, 0.5, 5)),
    "mandelbrot_zi_4_dyadic": dict(d=("zi", -2.0, 2.0, 4)),
    "cut_inside": dict(d=("cr", -0.9, 0.0, 5)),
    "hologram_row_7": dict(d=(plot.rotate(plot.IDENTITY, "zr", "ci", 37.0)[0], -0.9, 1.3, 7), projection=plot.HOLOGRAM),
    "ship": dict(d=("zi", -1.5, 1.2, 3), ship=True),
    "power_3": dict(d=("cr", -1.0, 1.0, 7), degree=3),
    "tricorn": dict(d=("zr", -2.0, 0.5, 5), formula=1),
    "julia_z": dict(d=("zi", -1.0, 1.1, 6), c=(-0.8, 0.156)),
    "256_slices": dict(d=("zr", -2.0, 2.0, 256)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_planes_are_the_weighted_sums_of_the_depth_renders_planes(ref, oracle, case):
    kw = dict(CASES[case])
    d = kw.pop("d")
    lut = plot.demo_table(d[3]) + np.uint32(0x030201)  # every neighbour differs, no entry is all zero
    own = oracle.init_states(1337, 0, THREADS)
    planes, vc = plot.draw(ref, W, H, MAX, MIN, THREADS, LAUNCHES, depth=d, states=own, **kw)
    states = oracle.init_states(1337, 0, THREADS)
    hist, cnt = plot.draw(ref, W, H, MAX, MIN, THREADS, LAUNCHES, depth=d, lut=lut, states=states, **kw)
    assert vc["increments"] > 0 and sum(bool(p.any()) for p in planes) >= 2
    assert hist.shape == (3, H, W) and np.array_equal(hist, plot.combine(lut, planes))
    assert int(hist.sum()) == cnt["increments"] > vc["increments"]
    assert {k: v for k, v in cnt.items() if k != "increments"} == {k: v for k, v in vc.items() if k != "increments"}
    assert states.tobytes() == own.tobytes()


def test_a_one_hot_table_gives_that_slice(ref):
    d = ("cr", -2.0, 0.5, 5)
    planes, vc = plot.draw(ref, W, H, MAX, MIN, THREADS, LAUNCHES, depth=d)
    populated = [s for s in range(5) if planes[s].any()]
    assert len(populated) >= 2
    for s in populated[:2]:
        lut = np.zeros(5, dtype=np.uint32)
        lut[s] = 1
        hist, cnt = plot.draw(ref, W, H, MAX, MIN, THREADS, LAUNCHES, depth=d, lut=lut)
        assert np.array_equal(hist[0], planes[s]) and not hist[1].any() and not hist[2].any()
        assert cnt["increments"] == int(planes[s].sum()) and cnt["replay_steps"] == vc["replay_steps"]


def test_the_constant_table_gives_the_section_three_times(ref):
    d = ("ci", -0.3, 0.3, 1)
    planes, vc = plot.draw(ref, W, H, MAX, MIN, THREADS, LAUNCHES, depth=d)
    hist, cnt = plot.draw(ref, W, H, MAX, MIN, THREADS, LAUNCHES, depth=d, lut=[0x010101])
    assert planes[0].any() and all(np.array_equal(hist[j], planes[0]) for j in range(3))
    assert cnt["increments"] == 3 * vc["increments"]


def test_a_zero_entry_adds_nothing_and_only_increments_notices(ref):
    d = ("cr", -2.0, 0.5, 5)
    planes, vc = plot.draw(ref, W, H, MAX, MIN, THREADS, LAUNCHES, depth=d)
    s = int(np.argmax([int(p.sum()) for p in planes]))  # the fullest slice goes dark
    lut = np.array([0x0000ff, 0x00ff00, 0xff0000, 0x010203, 0x7f0001], dtype=np.uint32)
    lut[s] = 0xff000000  # bits 24-31 are not read: an entry without a weight
    hist, cnt = plot.draw(ref, W, H, MAX, MIN, THREADS, LAUNCHES, depth=d, lut=lut)
    lit = lut.copy()
    lit[s] = 0
    assert np.array_equal(hist, plot.combine(lit, planes))
    assert cnt["increments"] == int(hist.sum()) > 0
    assert {k: v for k, v in cnt.items() if k != "increments"} == {k: v for k, v in vc.items() if k != "increments"}
    assert int(planes[s].sum()) > 0 and any(planes[t].any() for t in range(5) if t != s)  # it had points, and others have


def test_result_does_not_depend_on_the_thread_count(ref, oracle):
    got = []
    lut = plot.demo_table(5) + np.uint32(1)
    for omp in (0, 4):
        states = oracle.init_states(1337, 0, 256)
        hist, cnt = plot.draw(ref, 33, 17, 300, 0, 256, [50, 7], depth=("cr", -2.0, 0.5, 5), lut=lut, omp_threads=omp,
                              states=states)
        got.append((hist, cnt, states.tobytes()))
    assert got[0][1]["increments"] > 100
    assert np.array_equal(got[0][0], got[1][0]) and got[0][1] == got[1][1] and got[0][2] == got[1][2]


# ---- 2. the definition by hand --------------------------------------------------------------------------------------------


def by_hand(d, lo, hi, lut):
    """The definition in Python's IEEE doubles: early-out, truncation, bounds, then the table without its unread bits."""
    n = len(lut)
    if d < lo:
        return None
    s = int((d - lo) / ((hi - lo) / float(n)))
    return int(lut[s]) & 0xFFFFFF if 0 <= s < n else None


@pytest.mark.parametrize("lo, hi, n", [(-2.0, 2.0, 4), (-2.0, 0.5, 5), (-0.02, 0.02, 1), (0.1, 0.7, 256)])
def test_planted_depths_at_slice_edges_take_the_entry_the_definition_says(ref, lo, hi, n):
    lut = (plot.demo_table(n) + np.uint32(0x010101)) | np.uint32(0xAB000000)  # neighbours differ; the top byte is noise
    assert len(set(int(v) & 0xFFFFFF for v in lut)) == n
    delta = (hi - lo) / float(n)
    dyadic = math.frexp(delta)[0] == 0.5
    assert plot.entry_of(ref, lo, lo, hi, lut) == int(lut[0]) & 0xFFFFFF
    assert plot.entry_of(ref, math.nextafter(lo, -math.inf), lo, hi, lut) is None
    for s in range(n):
        edge = lo + s * delta
        for d in (edge, math.nextafter(edge, -math.inf), math.nextafter(edge, math.inf)):
            assert plot.entry_of(ref, d, lo, hi, lut) == by_hand(d, lo, hi, lut), (s, d)
        assert plot.entry_of(ref, lo + (s + 0.5) * delta, lo, hi, lut) == int(lut[s]) & 0xFFFFFF
        if dyadic and s > 0:  # exact edges and quotients: the slice's entry begins at its edge, its neighbour's ends below
            # (how far below is the definition's to say: d - min is a rounded difference -- tests/test_depth_host.py's note)
            assert plot.entry_of(ref, edge, lo, hi, lut) == int(lut[s]) & 0xFFFFFF
            assert plot.entry_of(ref, edge - delta / 1024.0, lo, hi, lut) == int(lut[s - 1]) & 0xFFFFFF
    assert plot.entry_of(ref, hi, lo, hi, lut) == by_hand(hi, lo, hi, lut)
    if dyadic:
        assert plot.entry_of(ref, hi, lo, hi, lut) is None
    assert plot.entry_of(ref, math.nan, lo, hi, lut) is None


def test_weights_of_an_entry(ref):
    assert [int(ref.plot_weight(0xAA030201, j)) for j in range(3)] == [1, 2, 3]
    assert plot.weights([0x00FF00, 0x7F0001]).tolist() == [[0, 255, 0], [1, 0, 127]]


# ---- 3. the stops' table ----------------------------------------------------------------------------------------------


def table_by_hand(stops, n):
    """"Palette render", Stops -> table, with k read as a slice index."""
    out = []
    for k in range(n):
        if k <= stops[0][0]:
            rgb = stops[0][1:]
        elif k >= stops[-1][0]:
            rgb = stops[-1][1:]
        else:
            a, b = next((a, b) for a, b in zip(stops, stops[1:]) if a[0] <= k < b[0])
            span = b[0] - a[0]
            rgb = [(va * (b[0] - k) + vb * (k - a[0]) + span // 2) // span for va, vb in zip(a[1:], b[1:])]
        out.append(rgb[0] | rgb[1] << 8 | rgb[2] << 16)
    return np.array(out, dtype=np.uint32)


README_STOPS = [(0, 0x00, 0x00, 0x30), (128, 0xFF, 0x80, 0x00), (255, 0xFF, 0xFF, 0xFF)]


@pytest.mark.parametrize("n", [256, 64, 5, 1])
def test_the_table_of_n_entries_is_the_palettes_with_k_a_slice_index(cb, n):
    """What the binary builds for `--depth ...:N --depth-palette 0:000030,128:ff8000,255:ffffff`: cb_palette_from_stops
    with n_entries = N.  Stops at or above N shape the gradient below them and are never reached themselves, as stops at
    or above -m are for --palette."""
    lut = cb.palette_from_stops(README_STOPS, n)
    assert lut.dtype == np.uint32 and lut.shape == (n,) and np.array_equal(lut, table_by_hand(README_STOPS, n))
    assert int(lut[0]) == 0x300000 and not (lut >> 24).any()
    if n == 256:
        assert int(lut[128]) == 0x0080FF and int(lut[255]) == 0xFFFFFF and int(lut[64]) == table_by_hand(README_STOPS, 256)[64]
    assert np.array_equal(lut, cb.palette_from_stops(README_STOPS, 256)[:n])  # a prefix of the longer table


# ---- 4. the header and the package ------------------------------------------------------------------------------------


def test_header_section_and_names(cb, repo_root):
    import cudabrot_amd.capi as capi

    with open(os.path.join(repo_root, "include", "cudabrot_amd.h")) as f:
        text = f.read()
    assert text.index("---- Depth render:") < text.index("---- Depth-palette render:") < text.index("---- Renderer:")
    start = text.index("---- Depth-palette render:")
    section = text[start:text.index("---- Renderer:", start)]
    for phrase in ("n_entries == N", "R = bits 0-7, G = bits 8-15", "B = bits 16-23", "Unchanged from \"Depth render\"",
                   "adds weight_j(lut[s]) to its pixel of plane j", "increments is the sum of the weights added",
                   "cb_palette_from_stops(stops, n, lut, N)", "common maximum", "weight_j(lut[s]) * V[s]", "0x010101"):
        assert phrase in section, phrase
    names = ("cb_draw_buddhabrot_depth_palette", "cb_renderer_set_depth_palette", "cb_renderer_depth_palette",
             "cb_renderer_depth_palette_image")
    for name in names:
        assert name + "(" in text and name in capi.EXPORTED_SYMBOLS and hasattr(cb.lib, name)
    assert "20 the\n * depth-palette product kernel" in text and "21 the\n * depth-palette lock-step kernel" in text
    assert callable(cb.draw_buddhabrot_depth_palette)
    assert all(hasattr(cb.Renderer, n) for n in ("set_depth_palette", "depth_palette", "depth_palette_image"))
    assert cb.lib.cb_abi_version() == 1  # the change only adds


# ---- 5. validation that needs no device -------------------------------------------------------------------------------

NAN = math.nan


def call(cb, d, lut=4096, n_entries=None, *, variant=None, julia=None, projection=None, hist=4096, states=4096):
    """cb_draw_buddhabrot_depth_palette with pointers that are never followed: the lock-step variant consults no interior
    map, and a launch of no threads launches nothing, so an accepted call returns 0 without touching a device."""
    dims = cb.FractalDimensions.make(16, 16)
    it = cb.IterationControl(100, 20)
    p = (C.c_double * 8)(*(cb.IDENTITY_PROJECTION if projection is None else projection))
    c = None if julia is None else (C.c_double * 2)(*julia)
    n = (d.slices if d is not None else 1) if n_entries is None else n_entries
    return cb.lib.cb_draw_buddhabrot_depth_palette(C.byref(dims), hist, C.byref(it), p, c, None if d is None else C.byref(d),
                                                   lut, n, states, 0, 50, None,
                                                   cb.CB_KERNEL_SIMPLE if variant is None else variant, None)


def test_a_valid_call_is_accepted(cb):
    assert call(cb, cb.Depth.make("cr", -2.0, 0.5, 64)) == 0
    assert call(cb, cb.Depth.make("cr", -2.0, 0.5, 256)) == 0
    assert call(cb, cb.Depth.make("zi", -2.0, 2.0, 1), julia=(-0.8, 0.156)) == 0
    for flag in (cb.CB_KERNEL_POWER(3), cb.CB_KERNEL_FORMULA("tricorn"), cb.CB_KERNEL_FLAG_BURNING_SHIP):
        assert call(cb, cb.Depth.make("zi", -2.0, 2.0, 4), variant=cb.CB_KERNEL_SIMPLE | flag) == 0


def test_what_the_definition_and_the_depth_draw_refuse_is_refused(cb):
    good = cb.Depth.make("cr", -2.0, 0.5, 5)
    assert call(cb, good, lut=None) == INVALID  # no table
    for n in (0, 4, 6, 256):
        assert call(cb, good, n_entries=n) == INVALID, n  # a table of another length than N
    assert call(cb, None) == INVALID
    for bad in (((NAN, 0, 0, 0), 0.0, 1.0, 1), ("cr", NAN, 1.0, 1), ("cr", 1.0, 1.0, 1), ("cr", 1.0, 0.0, 1), ("cr", 0.0, 1.0, 0),
                ("cr", 0.0, 1.0, 257), ("cr", -1.7e308, 1.7e308, 1)):
        assert call(cb, cb.Depth.make(*bad)) == INVALID, bad
    assert call(cb, good, projection=(1, 0, 0, 0, 0, NAN, 0, 0)) == INVALID
    assert call(cb, good, julia=(2.5, 0.0)) == INVALID and call(cb, good, julia=(0.0, NAN)) == INVALID
    for variant in (cb.CB_KERNEL_TIMED, cb.CB_KERNEL_FULL_ITERATE, cb.CB_KERNEL_SIMPLE | cb.CB_KERNEL_FLAG_ANTI,
                    cb.CB_KERNEL_SIMPLE | cb.CB_KERNEL_FLAG_DRAIN, cb.CB_KERNEL_SIMPLE | (2 << 12), cb.CB_KERNEL_SIMPLE | (6 << 16),
                    cb.CB_KERNEL_SIMPLE | cb.CB_KERNEL_POWER(3) | cb.CB_KERNEL_FLAG_BURNING_SHIP,
                    cb.CB_KERNEL_SIMPLE | cb.CB_KERNEL_POWER(3) | cb.CB_KERNEL_FORMULA(1)):
        assert call(cb, good, variant=variant) == INVALID, hex(variant)
    assert call(cb, good, hist=None) == INVALID and call(cb, good, states=None) == INVALID
    assert cb.lib.cb_renderer_set_depth_palette(None, C.byref(good), 4096, 5) == INVALID
    assert cb.lib.cb_renderer_depth_palette(None, None, None) == 0
    assert cb.lib.cb_renderer_depth_palette_image(None, 1.0, 0, None, None, None) == INVALID
