"""The period-palette render (include/cudabrot_amd.h, "Period-palette render") on the GPU:

  1. three ways -- the product kernel (cb_debug_last_draw_kernel 28), the lock-step kernel (29), the CPU restatement
     (tests/period_reference.c) -- bit for bit on the three planes, generator states and every counter but skipped_steps,
     and the product's skipped_steps is the compressed restatement's, to the step; every case asserts, from the
     restatement's class counts, that the classes it is meant to exercise are non-empty, and the ten together reach all of
     (a) .. (f);
  2. the anchors: the constant table against the bounded render's kernels 26 and 27, and the one-hot sum;
  3. consecutive launches add up;
  4. everything the ABI refuses, with nothing written;
  5. the renderer: its column, what a period-palette renderer refuses, the renderer against the entry point, its image;
  6. the binary.
"""

import ctypes as C
import json
import os

import numpy as np
import pytest

import period_reference as period
import plot_harness
import plot_reference as plot
from bounded_harness import MAX, MIN, THREADS, bounded_launches
from conftest import read_state_file
from period_harness import KEYS, LOCKSTEP, NOT_INCREMENTS, PRODUCT, period_launches, pref, shape_of, three_ways  # noqa: F401
from plot_harness import INVALID, SAME, exe  # noqa: F401
from plot_harness import gpu_run as run
from test_gpu_renderer_kinds import getters, library_planes, make

pytestmark = pytest.mark.gpu

CROP = (-1.5, 0.7, -0.9, 1.1)
# the z_re, z_im plane turned by three angles: two unit rows with four irrational entries each
ROTATED = plot.rotate(plot.rotate(plot.rotate(plot.IDENTITY, "zr", "zi", 25.0), "zr", "cr", 40.0), "zi", "ci", 55.0)
RABBIT = (-0.123, 0.745)
GRADIENT = period.gradient_table(256)


def without(table, *entries):
    out = table.copy()
    out[list(entries)] = 0
    return out


# name: (the table, eps, what shape_of takes, the classes the restatement must count).  The classes were counted on the
# restatement when the cases were chosen (DESIGN.md 4.22 has the figures); a case whose class is empty is moved, not skipped.
CASES = {
    # the cardioid (period 1) is not replayed
    "reference_zr_zi": (without(GRADIENT, 1), period.DEFAULT_EPS, dict(box=CROP),
                        ("cycle_period", "tol_period", "tol_none", "zero_entry")),
    "ship_zr_cr": (GRADIENT, period.DEFAULT_EPS, dict(ship=True, projection=plot.ZR_CR, box=CROP),
                   ("cycle_period", "tol_period", "tol_none")),
    "cubic_rotated_exact": (GRADIENT, 0.0, dict(degree=3, projection=ROTATED, box=CROP),
                            ("cycle_period", "tol_period", "tol_none")),
    "tricorn_cr_ci_j1": (period.gradient_table(2), period.DEFAULT_EPS, dict(formula="tricorn", projection=plot.C_PLANE),
                         ("cycle_period", "cycle_none", "tol_period", "tol_none")),
    # every cycle the schedule finds by M = 120 is found at k = M with remainder 0; the orbits without a period are not replayed
    "reference_cr_ci_max_120": (without(GRADIENT, 0), period.DEFAULT_EPS, dict(max_iter=120, projection=plot.C_PLANE),
                                ("cycle_period", "tol_period", "tol_none", "rem_zero", "zero_entry")),
    # J = 1: the period-2 bulb's exact cycles have no period
    "reference_zr_cr_j1": (period.gradient_table(2), period.DEFAULT_EPS, dict(projection=plot.ZR_CR, box=CROP),
                           ("cycle_period", "cycle_none", "tol_period", "tol_none")),
    "julia_basilica": (GRADIENT, period.DEFAULT_EPS, dict(c=(-1.0, 0.0)), ("cycle_period",)),
    "julia_rabbit_zr_cr_exact": (GRADIENT, 0.0, dict(c=RABBIT, projection=plot.ZR_CR), ("cycle_period",)),
    # the rabbit's slowest orbits are not yet on an exact cycle at k = 60, and -m 130 ends before the next comparison
    "julia_rabbit_max_130": (GRADIENT, period.DEFAULT_EPS, dict(c=RABBIT, max_iter=130), ("cycle_period", "tol_period")),
    "julia_basilica_j1": (period.gradient_table(2), period.DEFAULT_EPS, dict(c=(-1.0, 0.0), box=CROP), ("cycle_none",)),
}


# ---- 1. three ways, on inputs that reach the paths -----------------------------------------------------------------------


@pytest.fixture(scope="module")
def cases(cb, pref, oracle):  # noqa: F811
    """Every case three ways, once for the module."""
    done = {}

    def get(name):
        if name not in done:
            lut, eps, kw, _ = CASES[name]
            done[name] = three_ways(cb, pref, oracle, lut, eps, **kw)
        return done[name]

    return get


@pytest.mark.parametrize("name", list(CASES))
def test_three_ways(cases, name):
    want, wc, extra, product = cases(name)
    assert wc["recorded"] > 0 and wc["increments"] > 0 and all(want[j].any() for j in range(3))
    assert extra["escaped"] > 0 and product["skipped_steps"] > 0
    for key in CASES[name][3]:
        assert extra[key] > 0, (key, extra)


def test_the_ten_cases_together_reach_every_class(cases):
    total = dict.fromkeys(period.CLASSES, 0)
    for name in CASES:
        for key in total:
            total[key] += cases(name)[2][key]
    assert all(v > 0 for v in total.values()), total


def test_a_fixed_c_on_zr_cr_is_one_row(cases):
    want = cases("julia_rabbit_zr_cr_exact")[0]
    rows = np.flatnonzero(want.sum(axis=(0, 2)))
    assert len(rows) == 1  # v = c_re for every point


# ---- 2. the anchors --------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,kw", [("reference_zr_cr", dict(projection=plot.ZR_CR, box=CROP)),
                                     ("tricorn", dict(formula="tricorn", box=CROP)),
                                     ("rabbit", dict(c=RABBIT, box=CROP))])
def test_the_constant_table_is_the_bounded_render_three_times(cb, name, kw):
    for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
        want, wc, kernel, states = bounded_launches(cb, base, **kw)
        assert kernel == 26 + base and wc["recorded"] > 0
        for n in (2, 256):
            hist, cnt, launched, after = period_launches(cb, base, period.constant_table(n), **kw)
            assert launched == PRODUCT + base and cnt["status"] == 0
            for j in range(3):
                assert np.array_equal(hist[j], want), (base, n, j)
            assert np.array_equal(after, states)
            assert cnt["increments"] == 3 * wc["increments"] > 0
            assert {k: cnt[k] for k in NOT_INCREMENTS} == {k: wc[k] for k in NOT_INCREMENTS}
            assert cnt["skipped_steps"] == wc["skipped_steps"]  # the same schedule: the same steps saved, none for a colour


def test_the_one_hot_tables_sum_to_the_bounded_render(cb):
    n, kw = 5, dict(box=CROP)  # J = 4: periods 0 .. 4
    want, wc, _, states = bounded_launches(cb, cb.CB_KERNEL_DEFAULT, **kw)
    parts = []
    for k in range(n):
        hist, cnt, launched, after = period_launches(cb, cb.CB_KERNEL_DEFAULT, period.one_hot(n, k), **kw)
        assert launched == PRODUCT and cnt["status"] == 0 and np.array_equal(after, states)
        assert not hist[1].any() and not hist[2].any() and int(hist[0].sum()) == cnt["increments"]
        assert {x: cnt[x] for x in NOT_INCREMENTS} == {x: wc[x] for x in NOT_INCREMENTS}
        parts.append(hist[0])
    assert np.array_equal(sum(parts), want)
    assert all(p.any() for p in parts[:3])  # no period, the cardioid, the bulb
    lut = period.gradient_table(n)
    hist = period_launches(cb, cb.CB_KERNEL_DEFAULT, lut, **kw)[0]
    for j in range(3):
        assert np.array_equal(hist[j], sum(np.uint64((int(e) >> (8 * j)) & 255) * p for e, p in zip(lut, parts)))


# ---- 3. launches add up ----------------------------------------------------------------------------------------------------


def test_consecutive_launches_equal_one_launch_of_the_sum(cb):
    for kw in (dict(projection=ROTATED, box=CROP), dict(c=RABBIT, projection=plot.HOLOGRAM)):
        for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
            a = period_launches(cb, base, without(GRADIENT, 2), launches=(3, 50, 1), **kw)
            b = period_launches(cb, base, without(GRADIENT, 2), launches=(54,), **kw)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3])
            assert {k: a[1][k] for k in KEYS} == {k: b[1][k] for k in KEYS}
            assert a[1]["recorded"] > 0 and a[1]["increments"] > 0


def test_min_escape_iterations_is_not_read(cb):
    for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
        a = period_launches(cb, base, GRADIENT, min_iter=0, launches=(20,))
        b = period_launches(cb, base, GRADIENT, min_iter=MAX + 100, launches=(20,))
        assert np.array_equal(a[0], b[0]) and {k: a[1][k] for k in KEYS} == {k: b[1][k] for k in KEYS}
        assert a[1]["increments"] > 0


# ---- 4. what the ABI refuses -----------------------------------------------------------------------------------------------


def test_period_launches_refuse_what_they_do_not_define(cb):
    import torch

    threads = 256
    dims = cb.FractalDimensions.make(64, 64)
    it = cb.IterationControl(100, 20)
    bufs = plot_harness.Launches(cb, dims, threads, planes=3, tables={"lut": GRADIENT})
    buf, states, counters, table = bufs.out, bufs.states, bufs.counters, bufs.tables["lut"]
    torch.cuda.synchronize()
    before = states.cpu().numpy().copy()
    good = (C.c_double * 8)(*cb.IDENTITY_PROJECTION)
    c_good = (C.c_double * 2)(-1.0, 0.0)
    d, b, i, s = C.byref(dims), buf.data_ptr(), C.byref(it), states.data_ptr()

    def draw(variant=0, c=None, m=good, samples=5, lut=table.data_ptr(), n=256, eps=period.DEFAULT_EPS):
        return cb.lib.cb_draw_buddhabrot_periods(d, b, i, m, c, lut, n, eps, s, threads, samples, counters.data_ptr(), variant,
                                                 None)

    nan, inf = float("nan"), float("inf")
    power3, tricorn, ship = cb.CB_KERNEL_POWER(3), cb.CB_KERNEL_FORMULA(1), cb.CB_KERNEL_FLAG_BURNING_SHIP
    # the table and the tolerance
    assert draw(lut=None) == INVALID
    for n in (0, 1, 1025, 1 << 24):
        assert draw(n=n) == INVALID, n
    for eps in (-1.0, -5e-324, inf, -inf, nan):
        assert draw(eps=eps) == INVALID, eps
    # what cb_draw_buddhabrot_bounded refuses
    flags = [cb.CB_KERNEL_FLAG_ANTI, cb.CB_KERNEL_FLAG_DRAIN, cb.CB_KERNEL_FLAG_ANTI | ship, power3 | ship,
             cb.CB_KERNEL_POWER(8) | ship, tricorn | ship, tricorn | power3, cb.CB_KERNEL_FORMULA(5) | cb.CB_KERNEL_POWER(8),
             tricorn | cb.CB_KERNEL_FLAG_ANTI, power3 | cb.CB_KERNEL_FLAG_DRAIN, 2 << 12, 9 << 12, 6 << 16]
    for flag in flags:
        for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
            for c in (None, c_good):
                assert draw(base | flag, c=c) == INVALID, (base, flag)
    for variant in (cb.CB_KERNEL_TIMED, cb.CB_KERNEL_FULL_ITERATE, cb.CB_KERNEL_TIMED | ship, cb.CB_KERNEL_FULL_ITERATE | power3):
        for c in (None, c_good):
            assert draw(variant, c=c) == INVALID, variant
    for c in ((2.5, 0.0), (0.0, -2.0000001), (nan, 0.0), (0.0, nan), (0.0, inf), (-inf, 0.0)):
        for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
            assert draw(base, c=(C.c_double * 2)(*c)) == INVALID, c
    for j in range(8):
        for bad in (nan, inf):
            m = list(cb.IDENTITY_PROJECTION)
            m[j] = bad
            assert draw(m=(C.c_double * 8)(*m)) == INVALID
    assert draw(m=None) == INVALID
    t, e, cp = table.data_ptr(), period.DEFAULT_EPS, counters.data_ptr()
    assert cb.lib.cb_draw_buddhabrot_periods(None, b, i, good, None, t, 256, e, s, threads, 5, cp, 0, None) == INVALID
    assert cb.lib.cb_draw_buddhabrot_periods(d, None, i, good, None, t, 256, e, s, threads, 5, cp, 0, None) == INVALID
    assert cb.lib.cb_draw_buddhabrot_periods(d, b, None, good, None, t, 256, e, s, threads, 5, cp, 0, None) == INVALID
    assert cb.lib.cb_draw_buddhabrot_periods(d, b, i, good, None, t, 256, e, None, threads, 5, cp, 0, None) == INVALID
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0 and int(counters.sum()) == 0
    assert np.array_equal(states.cpu().numpy(), before)
    # no threads or no samples: nothing launched, success
    assert draw(samples=0) == 0
    assert cb.lib.cb_draw_buddhabrot_periods(d, b, i, good, None, t, 256, e, s, 0, 5, cp, 0, None) == 0
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0 and np.array_equal(states.cpu().numpy(), before)
    # every variant cb_draw_buddhabrot_bounded accepts, with either source; the bounds of c, n_entries and eps are allowed
    accepted = [0, ship, tricorn, cb.CB_KERNEL_FORMULA(5)] + [cb.CB_KERNEL_POWER(deg) for deg in range(3, 9)]
    n = 0
    for flag in accepted:
        for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
            for c in (None, c_good, (C.c_double * 2)(2.0, -2.0)):
                assert draw(base | flag, c=c) == 0, (base, flag)
                n += 1
    for entries, eps in ((2, 0.0), (256, 1.7976931348623157e308)):
        assert draw(n=entries, eps=eps) == 0
        n += 1
    torch.cuda.synchronize()
    cnt = bufs.read_counters()
    assert cnt["samples"] == n * 5 * threads and cnt["status"] == 0 and cnt["rejected"] == 0
    assert int(buf.sum()) == cnt["increments"] > 0


# ---- 5. the renderer -------------------------------------------------------------------------------------------------------

# cb_renderer_set_period_palette on the starting renderers of tests/test_gpu_renderer_kinds.py: 1 accepted, 0 refused --
# literal data: cb_renderer_set_bounded's column
PERIOD_COLUMN = {
    "plain": 1,
    "channels": 0,
    "focused": 0,
    "projected": 1,
    "julia": 1,
    "plain + palette": 0,
    "projected + palette": 0,
    "julia + palette": 0,
    "projected + depth": 0,
    "julia + depth palette": 0,
    "projected + frames": 0,
    "julia + phoenix": 0,
    "plain after a pass": 0,
    "projected after a pass": 0,
}
TABLE8 = np.ascontiguousarray(period.gradient_table(8), dtype=np.uint32)


def set_pp(cb, r, lut=TABLE8, n=None, eps=period.DEFAULT_EPS):
    return cb.lib.cb_renderer_set_period_palette(r._h, None if lut is None else lut.ctypes.data, len(lut) if n is None else n,
                                                 eps)


@pytest.mark.parametrize("name", list(PERIOD_COLUMN))
def test_set_period_palette_on_every_starting_renderer(cb, name):
    accepted = PERIOD_COLUMN[name]
    with make(cb, name, name == "focused") as r:
        h, w = r.dims.h, r.dims.w
        before, hist = getters(r), r.read_histogram()
        assert r.period_palette() is None
        code = set_pp(cb, r)
        if not accepted:
            assert code == INVALID and r.period_palette() is None and not r.bounded()
            assert getters(r) == before
            after = r.read_histogram()
            assert after.shape == hist.shape and np.array_equal(after, hist)
            assert library_planes(cb, r) == (hist.shape[0] if hist.ndim == 3 else 1)
            return
        assert code == 0 and r.period_palette() == (8, period.DEFAULT_EPS) and not r.bounded()
        # the source of c stays; a plain renderer gains the identity, as with a palette
        now = getters(r)
        assert now[1:] == before[1:] and np.ravel(now[0]).tolist() == list(cb.IDENTITY_PROJECTION)
        assert r.read_histogram().shape == (3, h, w) and library_planes(cb, r) == 3
        assert set_pp(cb, r) == INVALID  # once
        r.render_passes(1)
        assert cb.lib.cb_debug_last_draw_kernel() == PRODUCT and cb.lib.cb_renderer_interior_map_level(r._h) == 0
        cnt = r.read_counters().as_dict()
        assert int(r.read_histogram().sum()) == cnt["increments"] and cnt["status"] == 0 and cnt["rejected"] == 0
        assert cnt["increments"] > 0 and cnt["recorded"] > 0


def test_a_period_palette_renderer_takes_valid_arguments_only_and_refuses_every_setter_afterwards(cb):
    dims, it = cb.FractalDimensions.make(16, 16), cb.IterationControl(100, 20)
    good = (C.c_double * 8)(*cb.IDENTITY_PROJECTION)
    c_good = (C.c_double * 2)(-1.0, 0.0)
    p_good = (C.c_double * 2)(-0.5, 0.0)
    depth = cb.Depth.make("cr", -2.0, 0.5, 4)
    table = np.ascontiguousarray(plot.demo_table(100), dtype=np.uint32)
    slice_table = np.ascontiguousarray(plot.demo_table(4), dtype=np.uint32)
    frames = np.ascontiguousarray([cb.IDENTITY_PROJECTION] * 2, dtype=np.float64)
    setters = {
        "focus": lambda r: cb.lib.cb_renderer_set_focus(r._h, 6, 2, 1, 0),
        "projection": lambda r: cb.lib.cb_renderer_set_projection(r._h, good),
        "julia": lambda r: cb.lib.cb_renderer_set_julia(r._h, good, c_good),
        "palette": lambda r: cb.lib.cb_renderer_set_palette(r._h, table.ctypes.data, table.size),
        "depth": lambda r: cb.lib.cb_renderer_set_depth(r._h, C.byref(depth)),
        "depth_palette": lambda r: cb.lib.cb_renderer_set_depth_palette(r._h, C.byref(depth), slice_table.ctypes.data, 4),
        "frames": lambda r: cb.lib.cb_renderer_set_frames(r._h, frames.ctypes.data, 2),
        "phoenix": lambda r: cb.lib.cb_renderer_set_phoenix(r._h, p_good),
        "bounded": lambda r: cb.lib.cb_renderer_set_bounded(r._h),
        "period_palette": lambda r: set_pp(cb, r),
    }
    nan, inf = float("nan"), float("inf")
    for start in ("plain", "projected", "julia"):
        with cb.Renderer(dims, it, device=0, n_threads=256) as r:
            if start == "projected":
                r.set_projection(plot.ZR_CR)
            elif start == "julia":
                r.set_julia((-1.0, 0.0), plot.ZR_CR)
            before = getters(r)
            # arguments that do not pass leave the renderer what it was
            high = TABLE8.copy()
            high[5] |= 0x01000000
            big = np.zeros(1025, dtype=np.uint32)
            for code in (set_pp(cb, r, None, 8), set_pp(cb, r, n=1), set_pp(cb, r, n=0), set_pp(cb, r, big), set_pp(cb, r, high),
                         set_pp(cb, r, eps=-1.0), set_pp(cb, r, eps=inf), set_pp(cb, r, eps=nan)):
                assert code == INVALID
            assert getters(r) == before and r.period_palette() is None and r.read_histogram().shape == (16, 16)
            r.set_period_palette(TABLE8, 0.0)
            assert r.period_palette() == (8, 0.0)
            before = getters(r)
            fresh = r.read_rng_states().copy()
            for name, setter in setters.items():
                assert setter(r) == INVALID, (start, name)
                assert getters(r) == before and r.period_palette() == (8, 0.0), (start, name)
            # render_passes and prepare take what the entry point takes
            for variant in (cb.CB_KERNEL_FLAG_ANTI, cb.CB_KERNEL_FLAG_DRAIN, cb.CB_KERNEL_FULL_ITERATE, cb.CB_KERNEL_TIMED,
                            cb.CB_KERNEL_POWER(3) | cb.CB_KERNEL_FLAG_BURNING_SHIP):
                assert cb.lib.cb_renderer_render_passes(r._h, 1, variant) == INVALID, variant
            hist = r.read_histogram()
            assert hist.shape == (3, 16, 16) and int(hist.sum()) == 0 and r.read_counters().as_dict()["samples"] == 0
            assert np.array_equal(r.read_rng_states(), fresh)
            # the images of the renders it is not stay refused, and its own refuses what the palette's does
            out = np.zeros((16, 16, 3), dtype=">u2")
            assert cb.lib.cb_renderer_palette_image(r._h, 1.0, 0, out.ctypes.data, None, None) == INVALID
            assert cb.lib.cb_renderer_depth_palette_image(r._h, 1.0, 0, out.ctypes.data, None, None) == INVALID
            assert cb.lib.cb_renderer_period_palette_image(r._h, 1.0, 0, None, None, None) == INVALID
            assert cb.lib.cb_renderer_period_palette_image(r._h, 1.0, 7, out.ctypes.data, None, None) == INVALID  # no such mode
            r.render_passes(1, cb.CB_KERNEL_FORMULA(1))  # and it renders, with a step of the plotted path
            assert cb.lib.cb_debug_last_draw_kernel() == PRODUCT
            assert int(r.read_histogram().sum()) == r.read_counters().as_dict()["increments"] > 0
    with cb.Renderer(dims, it, device=0, n_threads=256) as r:  # and the other renderers have no such image
        out = np.zeros((16, 16, 3), dtype=">u2")
        assert cb.lib.cb_renderer_period_palette_image(r._h, 1.0, 0, out.ctypes.data, None, None) == INVALID
        r.set_bounded()
        assert cb.lib.cb_renderer_period_palette_image(r._h, 1.0, 0, out.ctypes.data, None, None) == INVALID


def host_image(cb, hist, gamma):
    """"Palette render", Image, on the host: the three planes as one w x 3h image, then interleaved -> ([h, w, 3]
    big-endian u16, max, scale)."""
    planes, h, w = hist.shape
    gray, mx, scale = cb.set_grayscale_pixels(hist.reshape(3 * h, w), gamma)
    return np.ascontiguousarray(gray.reshape(3, h, w).transpose(1, 2, 0)).astype(">u2"), mx, scale


@pytest.mark.parametrize("base", [0, 1], ids=["product", "lockstep"])
@pytest.mark.parametrize("name", ["reference_zr_zi", "cubic_rotated_exact", "julia_rabbit_zr_cr_exact", "plain"])
def test_renderer_against_the_entry_point_on_identical_passes(cb, base, name):
    lut, eps, case = (GRADIENT, period.DEFAULT_EPS, dict(box=CROP)) if name == "plain" else CASES[name][:3]
    kw = shape_of(case)
    kw.update(launches=(50, 100))  # one pass, then two fused: the same samples per generator
    want, wc, kernel, states = period_launches(cb, base, lut, eps, **kw)
    variant = plot_harness.variant_of(cb, base, kw["degree"], kw["ship"], plot.code_of(kw["formula"]))
    dims = cb.FractalDimensions.make(kw["w"], kw["h"], *kw["box"])
    with cb.Renderer(dims, cb.IterationControl(MAX, MIN), device=0, n_threads=THREADS) as r:
        if name == "plain":
            pass  # set_period_palette alone brings the identity
        elif kw["c"] is None:
            r.set_projection(kw["projection"])
        else:
            r.set_julia(kw["c"], kw["projection"])
        assert r.period_palette() is None
        r.set_period_palette(lut, eps)
        assert r.period_palette() == (len(lut), eps) and r.julia() == (None if kw["c"] is None else tuple(kw["c"]))
        assert np.ravel(r.projection()).tolist() == plot.matrix(kw["projection"]).tolist()
        r.prepare(variant)  # must not fail
        r.render_passes(1, variant)
        r.finish()
        r.render_passes(2, variant)
        assert cb.lib.cb_debug_last_draw_kernel() == kernel == PRODUCT + base
        assert cb.lib.cb_renderer_interior_map_level(r._h) == 0
        hist = r.read_histogram()
        cnt = r.read_counters().as_dict()
        after = r.read_rng_states().view(np.uint32)
        assert hist.shape == (3, kw["h"], kw["w"])
        assert cnt["status"] == 0 and {k: cnt[k] for k in KEYS} == {k: wc[k] for k in KEYS}
        assert wc["recorded"] > 0 and np.array_equal(hist, want) and np.array_equal(after, states)
        # the image: the three planes under their common maximum, the palette image's arithmetic
        for gamma in (1.0, 2.2):
            rgb, mx, scale = r.period_palette_image(gamma)
            body, want_max, want_scale = host_image(cb, hist, gamma)
            assert mx == want_max == int(hist.max()) > 0 and scale == want_scale
            assert rgb.shape == (kw["h"], kw["w"], 3) and rgb.tobytes() == body.tobytes()
        # the buffer and the generators go out and come back as for a palette renderer
        r.write_histogram(hist)
        r.write_rng_states(r.read_rng_states())
        assert np.array_equal(r.read_histogram(), hist)


# ---- 6. the binary -------------------------------------------------------------------------------------------------------

CLI_W, CLI_H, CLI_MAX, CLI_MIN = 64, 48, 130, 10
STOPS = [(0, 0x40, 0x40, 0x40), (1, 0xFF, 0x00, 0x00), (2, 0x00, 0xFF, 0x00), (3, 0x00, 0x00, 0xFF), (8, 0xFF, 0xFF, 0x00)]
STOPS_TEXT = "0:404040,1:ff0000,2:00ff00,3:0000ff,8:ffff00"
CLI_COMMON = ["--bounded", "--period-palette", STOPS_TEXT, "-w", str(CLI_W), "-h", str(CLI_H), "-m", str(CLI_MAX), "-c",
              str(CLI_MIN)]


def api_render(cb, passes, variant=0, c=None, projection=None, eps=None, gamma=None):
    """What the binary's run is: a renderer of its default threads and seed -> (hist, counters, PPM body or None)."""
    dims = cb.FractalDimensions.make(CLI_W, CLI_H)
    lut = cb.palette_from_stops(STOPS, 9)  # the largest K given + 1
    with cb.Renderer(dims, cb.IterationControl(CLI_MAX, CLI_MIN), device=0) as r:
        if c is not None:
            r.set_julia(c, projection)
        elif projection is not None:
            r.set_projection(projection)
        if eps is None:
            r.set_period_palette(lut)
            assert r.period_palette() == (9, 2.0 ** -66)  # the binary's default
        else:
            r.set_period_palette(lut, eps)
        r.render_passes(passes, variant)
        body = None if gamma is None else r.period_palette_image(gamma)[0]
        return r.read_histogram(), r.read_counters().as_dict(), body


def read_ppm(path, w, h):
    with open(path, "rb") as f:
        data = f.read()
    header = b"P6\n%d %d\n65535\n" % (w, h)
    assert data[:len(header)] == header and len(data) == len(header) + 6 * w * h  # one P6 of w x h, 16 bits
    return np.frombuffer(data, dtype=">u2", offset=len(header)).reshape(h, w, 3)


@pytest.fixture(scope="module")
def three_passes(cb):
    """Three passes of the binary's run through the API, once for the module -> (hist, counters, PPM body at -g 2.2)."""
    want, wc, body = api_render(cb, 3, gamma=2.2)
    assert cb.lib.cb_debug_last_draw_kernel() == PRODUCT and wc["recorded"] > 0 and wc["skipped_steps"] > 0
    assert all(want[j].any() for j in range(3))
    return want, wc, body


def test_cli_periods_equals_the_api_and_resumes(exe, tmp_path, three_passes):  # noqa: F811
    common, (want, wc, body) = CLI_COMMON, three_passes
    one_buf, one_side, one_ppm = str(tmp_path / "one.bin"), str(tmp_path / "one.rng"), str(tmp_path / "one.ppm")
    r = run(exe, "--passes", "3", "-s", one_buf, "--rng-state", one_side, "--stats", "-g", "2.2", "-o", one_ppm, *common)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Saving image." in r.stdout and "Done! Output image saved: %s" % one_ppm in r.stdout
    lines = r.stderr.strip().split("\n")
    assert [float.fromhex(v) for v in json.loads(lines[0])["projection"]] == [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]
    assert json.loads(lines[1]) == {"bounded": True}
    assert json.loads(lines[2]) == {"period_palette": [[0, "404040"], [1, "ff0000"], [2, "00ff00"], [3, "0000ff"], [8, "ffff00"]],
                                    "period_eps": "0x1p-66"}
    stats = json.loads(lines[-1])
    assert stats["status"] == 0 and {k: stats[k] for k in KEYS} == {k: wc[k] for k in KEYS}
    assert np.array_equal(read_state_file(one_buf, CLI_H, CLI_W, planes=3), want)
    assert read_ppm(one_ppm, CLI_W, CLI_H).tobytes() == body.tobytes()  # -o: one 16-bit PPM, the renderer's image
    # two passes, the two files written, then one more pass on them: the same run
    buf, side, ppm = str(tmp_path / "two.bin"), str(tmp_path / "two.rng"), str(tmp_path / "two.ppm")
    assert run(exe, "--passes", "2", "-s", buf, "--rng-state", side, "-o", os.devnull, *common).returncode == 0
    r2 = run(exe, "--passes", "1", "-s", buf, "--rng-state", side, "-g", "2.2", "-o", ppm, *common)
    assert r2.returncode == 0 and "Continuing the sample stream after 2 passes." in r2.stdout, r2.stdout
    for a, b in ((buf, one_buf), (side, one_side), (ppm, one_ppm)):
        with open(a, "rb") as fa, open(b, "rb") as fb:
            assert fa.read() == fb.read(), a


def test_cli_periods_selects_its_kernels_and_tone_maps_on_the_host_too(cb, exe, tmp_path, three_passes):  # noqa: F811
    common, (want, wc, body) = CLI_COMMON, three_passes
    # --kernel simple is the lock-step kernel (29): the same buffer and counters, and nothing skipped; the default is the
    # product kernel (28), whose compression shows in skipped_steps
    simple = str(tmp_path / "simple.bin")
    r3 = run(exe, "--kernel", "simple", "--passes", "3", "-s", simple, "--stats", "-o", os.devnull, *common)
    assert r3.returncode == 0, r3.stdout + r3.stderr
    stats3 = json.loads(r3.stderr.strip().split("\n")[-1])
    assert {k: stats3[k] for k in SAME} == {k: wc[k] for k in SAME} and stats3["skipped_steps"] == 0 < wc["skipped_steps"]
    assert np.array_equal(read_state_file(simple, CLI_H, CLI_W, planes=3), want)
    lock, lc, _ = api_render(cb, 3, cb.CB_KERNEL_SIMPLE)
    assert cb.lib.cb_debug_last_draw_kernel() == LOCKSTEP and lc["skipped_steps"] == 0 and np.array_equal(lock, want)
    # -c is not read, as under --bounded
    other = str(tmp_path / "c.bin")
    assert run(exe, "--passes", "3", "-s", other, "-o", os.devnull,
               *[a if a != str(CLI_MIN) else "120" for a in common]).returncode == 0
    assert np.array_equal(read_state_file(other, CLI_H, CLI_W, planes=3), want)
    # --tonemap host: the reference's host loop on the three planes as one image: the same bytes
    host_ppm = str(tmp_path / "host.ppm")
    assert run(exe, "--passes", "3", "--tonemap", "host", "-g", "2.2", "-o", host_ppm, *common).returncode == 0
    assert read_ppm(host_ppm, CLI_W, CLI_H).tobytes() == body.tobytes()


@pytest.mark.parametrize("flags,variant,c,projection,eps", [
    (["--plane", "cr,ci"], 0, None, plot.C_PLANE, None),
    (["--plane", "zr,cr", "--period-eps", "0"], 0, None, plot.ZR_CR, 0.0),
    (["--julia", "-1,0", "--plane", "zr,zi", "--rotate", "zi,cr:90"], 0, (-1.0, 0.0),
     ((1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0)), None),
    (["--julia", "0.3,0.5", "--period-eps", "0x1p-40", "--seed", "1337"], 0, (0.3, 0.5), None, 2.0 ** -40),
    (["--power", "3", "--plane", "zi,ci"], "power3", None, ((0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0)), None),
    (["--formula", "tricorn"], "tricorn", None, None, None),
    (["--burning-ship"], "ship", None, None, None),
], ids=["cr_ci", "zr_cr_exact", "julia_rotated", "julia_eps", "cubic_zi_ci", "tricorn", "ship"])
def test_cli_periods_with_the_flags_it_combines_with(cb, exe, tmp_path, flags, variant, c, projection, eps):  # noqa: F811
    variant = {0: 0, "power3": cb.CB_KERNEL_POWER(3), "tricorn": cb.CB_KERNEL_FORMULA(1),
               "ship": cb.CB_KERNEL_FLAG_BURNING_SHIP}[variant]
    buf = str(tmp_path / "b.bin")
    r = run(exe, *CLI_COMMON, *flags, "--passes", "1", "-s", buf, "--stats", "-o", os.devnull)
    assert r.returncode == 0, r.stdout + r.stderr
    assert '{"bounded": true}' in r.stderr.split("\n")
    said = [json.loads(line) for line in r.stderr.split("\n") if line.startswith('{"period_palette"')]
    assert len(said) == 1 and float.fromhex(said[0]["period_eps"]) == (2.0 ** -66 if eps is None else eps)
    want, wc, _ = api_render(cb, 1, variant, c=c, projection=projection, eps=eps)
    stats = json.loads(r.stderr.strip().split("\n")[-1])
    assert stats["status"] == 0 and {k: stats[k] for k in KEYS} == {k: wc[k] for k in KEYS}
    assert wc["recorded"] > 0 and wc["increments"] > 0
    assert np.array_equal(read_state_file(buf, CLI_H, CLI_W, planes=3), want)
