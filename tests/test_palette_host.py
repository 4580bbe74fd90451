"""The host side of the palette render (include/cudabrot_amd.h, "Palette render") without a GPU:

  1. cb_palette_from_stops against a restatement in Python integers;
  2. what it refuses;
  3. the tests' CPU restatement (tests/plot_reference.c) with a table against the same function without one -- two
     settings of the one restatement, which tests/test_julia_host.py pins to the definition either way;
  4. the names in the header and the package.
"""

import ctypes as C

import numpy as np
import pytest

import plot_reference as plot
from plot_harness import ref  # noqa: F401

INVALID = 1  # hipErrorInvalidValue


def table_of(stops, n):
    """The header's rule, in Python integers."""
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


SIXTEEN = [(3 * j * j + j, (37 * j) % 256, (255 - 16 * j) % 256, (j * j * 5) % 256) for j in range(16)]
STOPS = {
    "one_stop": ([(7, 1, 2, 3)], 20),
    "two_stops_rounding_half": ([(0, 0, 0, 0), (2, 1, 3, 255)], 4),  # k = 1: 0.5 -> 1, 1.5 -> 2, 127.5 -> 128
    "stops_at_0_and_n_minus_1": ([(0, 255, 0, 10), (99, 0, 255, 20)], 100),
    "stops_beyond_n": ([(5, 10, 20, 30), (1000, 250, 0, 130), (5000, 0, 0, 0)], 300),
    "first_stop_beyond_n": ([(50, 9, 8, 7), (60, 1, 1, 1)], 10),
    "sixteen_stops": (SIXTEEN, 800),
    "one_entry": ([(0, 5, 6, 7), (1, 9, 9, 9)], 1),
}


@pytest.mark.parametrize("name", list(STOPS))
def test_table_of_the_stops(cb, name):
    stops, n = STOPS[name]
    got = cb.palette_from_stops(stops, n)
    assert got.dtype == np.uint32 and got.shape == (n,)
    assert np.array_equal(got, table_of(stops, n)), name
    assert not np.any(got >> 24)
    for k, r, g, b in stops:  # a stop inside the table is met exactly
        if k < n:
            assert int(got[k]) == r | g << 8 | b << 16


def test_the_rounding_case_by_hand(cb):
    assert [int(v) for v in cb.palette_from_stops([(0, 0, 0, 0), (2, 1, 3, 255)], 4)] == [
        0, 1 | 2 << 8 | 128 << 16, 1 | 3 << 8 | 255 << 16, 1 | 3 << 8 | 255 << 16]


def test_a_long_table_does_not_overflow(cb):
    stops = [(0, 255, 255, 255), (cb.CB_PALETTE_MAX_ENTRIES - 1, 0, 255, 1)]
    got = cb.palette_from_stops(stops, cb.CB_PALETTE_MAX_ENTRIES)
    span = cb.CB_PALETTE_MAX_ENTRIES - 1
    for k in (0, 1, span // 2, span // 2 + 1, span - 1, span):
        want = [(va * (span - k) + vb * k + span // 2) // span for va, vb in ((255, 0), (255, 255), (255, 1))]
        assert int(got[k]) == want[0] | want[1] << 8 | want[2] << 16, k


REFUSED = {
    "equal_k": [(5, 0, 0, 0), (5, 1, 1, 1)],
    "descending_k": [(9, 0, 0, 0), (5, 1, 1, 1)],
    "negative_k": [(-1, 0, 0, 0), (5, 1, 1, 1)],
    "no_stops": [],
    "seventeen_stops": [(j, 0, 0, 0) for j in range(17)],
    "red_above_255": [(0, 256, 0, 0)],
    "green_above_255": [(0, 0, 256, 0)],
    "blue_above_255": [(0, 0, 0, 1000)],
    "negative_component": [(0, 0, -1, 0)],
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_stops_refused(cb, name):
    stops = REFUSED[name]
    arr = (cb.PaletteStop * max(len(stops), 1))(*[cb.PaletteStop(*s) for s in stops])
    out = np.full(10, 0xDEADBEEF, dtype=np.uint32)
    assert cb.lib.cb_palette_from_stops(arr, len(stops), out.ctypes.data, 10) == INVALID
    assert np.all(out == 0xDEADBEEF)  # untouched
    with pytest.raises(cb.CudabrotError):
        cb.palette_from_stops(stops, 10)


def test_sizes_and_pointers_refused(cb):
    one = (cb.PaletteStop * 1)(cb.PaletteStop(0, 1, 2, 3))
    out = np.zeros(4, dtype=np.uint32)
    assert cb.lib.cb_palette_from_stops(one, 1, out.ctypes.data, 0) == INVALID
    assert cb.lib.cb_palette_from_stops(one, 1, out.ctypes.data, cb.CB_PALETTE_MAX_ENTRIES + 1) == INVALID
    assert cb.lib.cb_palette_from_stops(None, 1, out.ctypes.data, 4) == INVALID
    assert cb.lib.cb_palette_from_stops(one, 1, None, 4) == INVALID
    assert cb.lib.cb_palette_from_stops(one, -1, out.ctypes.data, 4) == INVALID
    assert cb.lib.cb_palette_from_stops(one, 1, out.ctypes.data, 4) == 0 and np.all(out == 1 | 2 << 8 | 3 << 16)


# ---- 3. the restatement with a table against itself without one -----------------------------------------------------

W = H = 64
THREADS, MAX, MIN, LAUNCHES = 256, 200, 5, [3, 2]
WINDOWS = [(5, 20), (20, 80), (40, 200)]  # G and B overlap
C_JULIA = (-0.8, 0.156)


def with_table(ref, lut, **case):
    """-> (hist [3, h, w], counters, zero_entry_steps)."""
    extra = {}
    hist, cnt = plot.draw(ref, W, H, MAX, MIN, THREADS, LAUNCHES, lut=lut, extra=extra, **case)
    return hist, cnt, extra["zero_entry_steps"]


def plain(ref, c, ship, degree, max_iter, min_iter, projection):
    """The same render by the same restatement without a table: one plane of weight 1."""
    return plot.draw(ref, W, H, max_iter, min_iter, THREADS, LAUNCHES, c=c, ship=ship, degree=degree,
                     projection=projection)


CASES = {
    "mandelbrot": dict(c=None, ship=False, degree=2, projection=plot.IDENTITY),
    "mandelbrot_hologram": dict(c=None, ship=False, degree=2, projection=plot.HOLOGRAM),
    "ship": dict(c=None, ship=True, degree=2, projection=plot.IDENTITY),
    "julia": dict(c=C_JULIA, ship=False, degree=2, projection=plot.IDENTITY),
    "julia_degree3_zr_cr": dict(c=C_JULIA, ship=False, degree=3, projection=plot.ZR_CR),
    "julia_ship": dict(c=C_JULIA, ship=True, degree=2, projection=plot.HOLOGRAM),
}


@pytest.mark.parametrize("name", list(CASES))
def test_constant_table_is_the_plain_render_in_every_plane(ref, name):
    """Table against no table: two settings of the one restatement."""
    case = CASES[name]
    lut = np.full(MAX, 0x010101, dtype=np.uint32)
    hist, cnt, zero_steps = with_table(ref, lut, **case)
    want, wc = plain(ref, max_iter=MAX, min_iter=MIN, **case)
    assert wc["recorded"] > 0 and wc["increments"] > 0
    for j in range(3):
        assert np.array_equal(hist[j], want), (name, j)
    assert cnt["increments"] == 3 * wc["increments"] and zero_steps == 0
    assert {k: cnt[k] for k in cnt if k != "increments"} == {k: wc[k] for k in wc if k != "increments"}


@pytest.mark.parametrize("name", list(CASES))
def test_window_table_is_the_plain_render_of_each_window(ref, name):
    """Each plane against the render without a table at that window's -m and -c: two settings of the one restatement."""
    case = CASES[name]
    lut = plot.window_table(MAX, WINDOWS)
    hist, cnt, zero_steps = with_table(ref, lut, **case)
    total = 0
    for j, (lo, hi) in enumerate(WINDOWS):
        want, wc = plain(ref, max_iter=hi, min_iter=lo, **case)
        assert np.array_equal(hist[j], want), (name, j)
        total += wc["increments"]
    assert cnt["increments"] == total == int(hist.sum())
    # every accepted k lies in a window here, so no entry looked up is zero
    assert zero_steps == 0


def test_weights_scale_the_planes_and_zero_entries_are_counted(ref):
    lut = np.full(MAX, 255 | 2 << 16, dtype=np.uint32)  # R 255, G 0, B 2
    lut[50:] = 0
    hist, cnt, zero_steps = with_table(ref, lut)
    want, wc = plain(ref, None, False, 2, 50, MIN, plot.IDENTITY)  # the orbits with k < 50
    full, fc = plain(ref, None, False, 2, MAX, MIN, plot.IDENTITY)
    assert np.array_equal(hist[0], 255 * want) and not hist[1].any() and np.array_equal(hist[2], 2 * want)
    assert cnt["increments"] == 257 * wc["increments"]
    assert cnt["recorded"] == fc["recorded"] and cnt["replay_steps"] == fc["replay_steps"]
    assert zero_steps == fc["replay_steps"] - wc["replay_steps"] > 0


def test_bits_24_to_31_are_not_read(ref):
    lut = plot.demo_table(MAX)
    a = with_table(ref, lut)
    b = with_table(ref, lut | np.uint32(0xAB000000))
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]


# ---- 4. names ----------------------------------------------------------------------------------------------------------


def test_names_in_header_and_package(cb, repo_root):
    import os

    import cudabrot_amd.capi as capi

    with open(os.path.join(repo_root, "include", "cudabrot_amd.h")) as f:
        text = f.read()
    for name in ("cb_palette_from_stops", "cb_draw_buddhabrot_palette", "cb_renderer_set_palette", "cb_renderer_palette",
                 "cb_renderer_palette_image"):
        assert name + "(" in text and name in capi.EXPORTED_SYMBOLS and hasattr(cb.lib, name)
    assert "Palette render" in text and "CB_PALETTE_MAX_ENTRIES (1 << 24)" in text and "CB_PALETTE_MAX_STOPS 16" in text
    assert cb.CB_PALETTE_MAX_ENTRIES == 1 << 24 and cb.CB_PALETTE_MAX_STOPS == 16
    assert C.sizeof(cb.PaletteStop) == 16
    assert callable(cb.palette_from_stops) and callable(cb.draw_buddhabrot_palette)
    for name in ("set_palette", "palette", "palette_image"):
        assert hasattr(cb.Renderer, name)
