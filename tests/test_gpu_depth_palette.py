"""The depth-palette render (include/cudabrot_amd.h, "Depth-palette render") on the GPU:

  1. every case three ways -- the product kernel (cb_debug_last_draw_kernel 20), the lock-step kernel (21), the CPU
     restatement (tests/plot_reference.c) -- bit for bit on the three planes, the generator states and every
     counter but skipped_steps;
  2. against the depth render's entry point, which is proven against the CPU on its own: no restatement involved;
  3. the renderer, its refusals and its image;
  4. the binary.

The shape is tests/test_gpu_depth.py's, small on purpose: 64 x 48 (a transposed plane stride shows), 1000 threads (a
ragged last wave and workgroup -- the lanes past the last thread stage the table and meet the barrier like the others),
launches of 3, 50 and 1 samples on the same generators, -m 500 -c 20 (orbits cross several 60-step chunk boundaries).

Every table has a weight that is zero in a slice that receives points, and -- where the render has more than one slice
to offer -- at least two slices with different entries receive points: a plane swap or a constant lookup would not pass.
N = 1 and a Julia set on a c axis have one slice by their nature; there the entry's three weights differ and one is zero."""

import ctypes as C
import json
import os

import numpy as np
import pytest

import plot_harness
import plot_reference as plot
from conftest import read_state_file
from plot_harness import C_JULIA, DEPTH_SHAPE, INVALID, IRRATIONAL_ROW, NOT_INCREMENTS, SAME, SQUARE  # noqa: F401
from plot_harness import exe, omp_threads, planar_states, ref, variant_of  # noqa: F401
from plot_harness import gpu_run as run

pytestmark = pytest.mark.gpu

PRODUCT, LOCKSTEP = 20, 21
W, H, MAX, MIN, THREADS, LAUNCHES = DEPTH_SHAPE


def gradient(cb, n):
    """Three stops over the N slices, red to green to blue: every entry but the middle one lacks a colour, and neighbours
    differ wherever N > 1."""
    if n == 1:
        return np.array([0x0300FF], dtype=np.uint32)  # R 255, G 0, B 3
    assert n >= 3
    return cb.palette_from_stops([(0, 255, 0, 0), (n // 2, 0, 255, 0), (n - 1, 0, 7, 255)], n)


def sixteen_stops(cb):
    """256 entries from 16 stops, 17 slices apart, whose colours drop one component in turn."""
    stops = [(17 * i, (37 * i + 11) % 256 if i % 3 else 0, (91 * i + 5) % 256 if i % 3 != 1 else 0,
              (53 * i + 200) % 256 if i % 3 != 2 else 0) for i in range(16)]
    assert stops[-1][0] == 255
    return cb.palette_from_stops(stops, 256)


def gpu_launches(cb, d, lut, variant, c=None, projection=plot.IDENTITY):
    """plot_harness.gpu_launches at this suite's shape, d = (row, min, max, slices): through
    cb_draw_buddhabrot_depth_palette with a table -> hist [3, h, w]; lut None through cb_draw_buddhabrot_depth -> [slices,
    h, w]."""
    return plot_harness.gpu_launches(cb, W, H, SQUARE, MAX, MIN, THREADS, LAUNCHES, variant, c, None, projection, d, lut)


def three_ways(cb, ref, oracle, d, lut, **kw):
    """plot_harness.three_ways at this suite's shape -> (the restatement's histogram, its counters, the depth
    restatement's N planes)."""
    r = plot_harness.three_ways(cb, ref, oracle, (PRODUCT, LOCKSTEP), None, W, H, SQUARE, MAX, MIN, THREADS, LAUNCHES,
                                depth=d, lut=lut, **kw)
    return r.want, r.wc, r.extra["planes"]


def tells_planes_and_slices_apart(lut, planes):
    """Some weight is zero in a slice that receives points, and two slices with different entries receive points."""
    populated = [s for s in range(len(lut)) if planes[s].any()]
    w = plot.weights(lut)
    assert any((w[s] == 0).any() for s in populated) and any(w[s].any() for s in populated)
    assert len({int(lut[s]) & 0xFFFFFF for s in populated}) >= 2, populated


# ---- 1. three ways ------------------------------------------------------------------------------------------------------

CASES = {
    "mandelbrot_cr_5": dict(d=("cr", -2.0, 0.5, 5)),  # a non-dyadic delta_d (the division)
    "mandelbrot_zi_4_dyadic": dict(d=("zi", -2.0, 2.0, 4)),  # the reciprocal
    "mandelbrot_cr_inner": dict(d=("cr", -0.9, 0.0, 5)),  # cut inside the set: points fall outside at both ends
    "hologram_irrational_row": dict(d=(IRRATIONAL_ROW, -0.9, 1.3, 7), projection=plot.HOLOGRAM),
    "ship": dict(d=("zi", -1.5, 1.2, 3), ship=True),
    "power_3": dict(d=("cr", -1.0, 1.0, 7), degree=3),
    "tricorn": dict(d=("zr", -2.0, 0.5, 5), formula=1),
    "julia_z_axis": dict(d=("zi", -1.0, 1.1, 6), c=C_JULIA),
}


@pytest.mark.parametrize("name", list(CASES))
def test_product_lockstep_and_restatement_agree(cb, ref, oracle, name):
    kw = dict(CASES[name])
    d = kw.pop("d")
    lut = gradient(cb, d[3])
    want, wc, planes = three_ways(cb, ref, oracle, d, lut, **kw)
    assert wc["recorded"] > 0 and wc["increments"] > 0 and int(planes.sum()) < wc["replay_steps"]  # some points are dropped
    assert all(p.any() for p in want)
    tells_planes_and_slices_apart(lut, planes)
    if name == "mandelbrot_cr_inner":  # points beyond both ends of the window: the wider window holds more at either end
        wider = CASES["mandelbrot_cr_5"]["d"]
        outer, _ = plot.draw(ref, W, H, MAX, MIN, THREADS, LAUNCHES, depth=wider, omp_threads=omp_threads())
        edges = wider[1] + np.arange(wider[3] + 1) * ((wider[2] - wider[1]) / wider[3])
        assert sum(int(outer[s].sum()) for s in range(wider[3]) if edges[s + 1] <= d[1]) > 0
        assert sum(int(outer[s].sum()) for s in range(wider[3]) if edges[s] >= d[2]) > 0


def test_256_slices_read_every_slot_of_the_staged_table(cb, ref, oracle):
    lut = sixteen_stops(cb)
    assert len({int(v) for v in lut}) > 200
    # |z| of a visited point stays below 8 + 2 sqrt 2; the window [-2, 2) holds the set's bulk: 1/64 per slice
    want, wc, planes = three_ways(cb, ref, oracle, ("zr", -2.0, 2.0, 256), lut)
    tells_planes_and_slices_apart(lut, planes)
    populated = [s for s in range(256) if planes[s].any()]
    print("populated slices", len(populated), populated[0], populated[-1])
    assert len(populated) >= 200 and populated[0] < 8 and populated[-1] > 247  # both ends of the table are read


def test_one_slice(cb, ref, oracle):
    lut = gradient(cb, 1)
    want, wc, planes = three_ways(cb, ref, oracle, ("ci", -0.3, 0.3, 1), lut)
    assert planes[0].any() and np.array_equal(want[0], 255 * planes[0]) and not want[1].any()
    assert np.array_equal(want[2], 3 * planes[0])


def test_julia_on_a_c_axis_has_one_colour_or_none(cb, ref, oracle):
    """The depth of every point is that of the fixed c: all of them take one entry, or none is in depth."""
    lut = np.array([0x010000, 0x000200, 0x0300FF, 0x040404, 0x050000], dtype=np.uint32)
    want, wc, planes = three_ways(cb, ref, oracle, ("cr", -2.0, 0.5, 5), lut, c=C_JULIA)
    s = int((C_JULIA[0] + 2.0) / 0.5)  # 2: R 255, G 0, B 3
    assert int(planes[s].sum()) == int(planes.sum()) > 0
    assert [int(want[j].sum()) for j in range(3)] == [int(x) * int(planes[s].sum()) for x in plot.weights(lut)[s]]
    assert (plot.weights(lut)[s] == 0).any() and len(set(plot.weights(lut)[s].tolist())) == 3
    want, wc, _ = three_ways(cb, ref, oracle, ("ci", 0.2, 1.0, 3), gradient(cb, 3), c=C_JULIA)  # c_im is below the window
    assert wc["increments"] == 0 and wc["recorded"] > 0 and wc["replay_steps"] > 0
    # a row over both: K_d from the fixed c moves the window of z_im
    want, wc, planes = three_ways(cb, ref, oracle, ((0.0, 1.0, 0.5, -2.0), -1.0, 1.0, 4), gradient(cb, 4), c=C_JULIA)
    tells_planes_and_slices_apart(gradient(cb, 4), planes)


def test_bits_24_to_31_of_the_device_table_change_nothing(cb):
    d = ("cr", -2.0, 0.5, 5)
    lut = gradient(cb, 5)
    for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
        clean, cc, _, cs = gpu_launches(cb, d, lut, base)
        noisy, nc, _, ns = gpu_launches(cb, d, lut | np.uint32(0xA5000000), base)
        assert cc["increments"] > 0 and np.array_equal(clean, noisy) and cc == nc and np.array_equal(cs, ns)


# ---- 2. against the depth entry point ---------------------------------------------------------------------------------

AGAINST = {
    "mandelbrot": dict(d=("cr", -2.0, 0.5, 5)),
    "hologram_c_axis": dict(d=("ci", -1.0, 1.0, 8), projection=plot.HOLOGRAM),
    "power_3": dict(d=("zi", -1.5, 1.5, 6), degree=3),
    "julia": dict(d=("zi", -1.0, 1.1, 6), c=C_JULIA),
}


@pytest.fixture(scope="module")
def depth_planes(cb):
    """V of every case of AGAINST and either kernel, from cb_draw_buddhabrot_depth: computed once, never changed."""
    out = {}
    for name, case in AGAINST.items():
        kw = dict(case)
        d = kw.pop("d")
        degree = kw.pop("degree", 2)
        for base in (0, 1):
            planes, cnt, kernel, states = gpu_launches(cb, d, None, variant_of(cb, base, degree), **kw)
            assert kernel == 18 + base and cnt["status"] == 0
            planes.setflags(write=False)
            out[name, base] = (planes, cnt, states)
    return out


@pytest.mark.parametrize("base", [0, 1], ids=["product", "lockstep"])
@pytest.mark.parametrize("name", list(AGAINST))
def test_planes_are_the_weighted_sums_of_the_depth_renders_planes(cb, depth_planes, name, base):
    kw = dict(AGAINST[name])
    d = kw.pop("d")
    variant = variant_of(cb, base, kw.pop("degree", 2))
    planes, vc, v_states = depth_planes[name, base]
    lut = gradient(cb, d[3])
    tells_planes_and_slices_apart(lut, planes)
    hist, cnt, kernel, states = gpu_launches(cb, d, lut, variant, **kw)
    assert kernel == PRODUCT + base and cnt["status"] == 0
    assert np.array_equal(hist, plot.combine(lut, planes))
    assert cnt["increments"] == int(hist.sum()) > vc["increments"] > 0
    assert {k: cnt[k] for k in NOT_INCREMENTS} == {k: vc[k] for k in NOT_INCREMENTS}
    assert cnt["skipped_steps"] == vc["skipped_steps"]  # the same early-outs, the same map, nothing skipped for a colour
    assert np.array_equal(states, v_states)
    # the one-hot table gives V[s], for the fullest slice and a neighbour of it that has points
    order = sorted(range(d[3]), key=lambda s: -int(planes[s].sum()))[:2]
    for s in order:
        assert planes[s].any()
        one_hot = np.zeros(d[3], dtype=np.uint32)
        one_hot[s] = 1
        hist, cnt, _, _ = gpu_launches(cb, d, one_hot, variant, **kw)
        assert np.array_equal(hist[0], planes[s]) and not hist[1].any() and not hist[2].any()
        assert cnt["increments"] == int(planes[s].sum())


@pytest.mark.parametrize("base", [0, 1], ids=["product", "lockstep"])
@pytest.mark.parametrize("c", [None, C_JULIA], ids=["projected", "julia"])
def test_the_constant_table_with_one_slice_is_the_section_three_times(cb, c, base):
    d = ("zi", -0.3, 0.3, 1)
    planes, vc, _, v_states = gpu_launches(cb, d, None, base, c, plot.HOLOGRAM)
    hist, cnt, kernel, states = gpu_launches(cb, d, [0x010101], base, c, plot.HOLOGRAM)
    assert kernel == PRODUCT + base and 0 < vc["increments"] < vc["replay_steps"]
    assert all(np.array_equal(hist[j], planes[0]) for j in range(3)) and cnt["increments"] == 3 * vc["increments"]
    assert {k: cnt[k] for k in NOT_INCREMENTS} == {k: vc[k] for k in NOT_INCREMENTS} and np.array_equal(states, v_states)


# ---- 3. the renderer ------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("base", [0, 1], ids=["product", "lockstep"])
@pytest.mark.parametrize("kind", ["projected", "julia_power_3"])
def test_renderer_resumed_from_its_files_equals_one_run(cb, ref, oracle, base, kind):
    c, degree = ((0.4, 0.0), 3) if kind == "julia_power_3" else (None, 2)
    d = ("zi", -1.0, 1.1, 6)
    lut = gradient(cb, 6)
    variant = variant_of(cb, base, degree)
    dims = cb.FractalDimensions.make(W, H)
    it = cb.IterationControl(300, 10)

    def renderer():
        r = cb.Renderer(dims, it, device=0, n_threads=THREADS)
        if c is None:
            r.set_projection(plot.HOLOGRAM)
        else:
            r.set_julia(c, plot.HOLOGRAM)
        assert r.depth_palette() is None
        r.set_depth_palette(d, lut)
        return r

    with renderer() as one:
        one.prepare(variant)  # must not fail
        one.render_passes(3, variant)
        assert cb.lib.cb_debug_last_draw_kernel() == PRODUCT + base
        want, wc, want_states = one.read_histogram(), one.read_counters().as_dict(), one.read_rng_states().copy()
        # the getter round-trips; the renderer is neither a palette renderer nor one with a depth
        got_depth, n = one.depth_palette()
        assert got_depth.as_tuple() == ((0.0, 1.0, 0.0, 0.0), -1.0, 1.1, 6) and n == 6
        raw, raw_n = cb.Depth(), C.c_uint32(77)
        assert cb.lib.cb_renderer_depth_palette(one._h, C.byref(raw), C.byref(raw_n)) == 1
        assert raw.as_tuple() == got_depth.as_tuple() and raw_n.value == 6
        assert cb.lib.cb_renderer_depth_palette(one._h, None, None) == 1
        assert one.depth() is None and one.palette() is None
    with renderer() as first:
        first.render_passes(2, variant)
        hist, states = first.read_histogram(), first.read_rng_states().copy()
    assert hist.shape == (3, H, W)
    with renderer() as second:
        second.write_histogram(hist)
        second.write_rng_states(states)
        with pytest.raises(ValueError):
            second.write_histogram(hist[0])
        second.render_passes(1, variant)
        got, got_states = second.read_histogram(), second.read_rng_states()
    assert wc["status"] == 0 and wc["increments"] > 100 and int(want.sum()) == wc["increments"]
    assert np.array_equal(got, want) and np.array_equal(got_states, want_states)
    st = oracle.init_states(1337, 0, THREADS)
    ref_hist, rc = plot.draw(ref, W, H, 300, 10, THREADS, [150], depth=d, lut=lut, projection=plot.HOLOGRAM, degree=degree,
                             c=c, omp_threads=omp_threads(), states=st)
    assert np.array_equal(want, ref_hist) and {k: wc[k] for k in SAME} == rc
    assert np.array_equal(want_states.view(np.uint32), planar_states(st))


def test_renderer_refuses_a_depth_palette_where_it_is_not_defined(cb):
    dims = cb.FractalDimensions.make(64, 64)
    it = cb.IterationControl(100, 20)
    good = (C.c_double * 8)(*cb.IDENTITY_PROJECTION)
    c_good = (C.c_double * 2)(*C_JULIA)
    d = cb.Depth.make("cr", -2.0, 0.5, 5)
    lut = np.array([0x0000FF, 0x00FF00, 0xFF0000, 0x010203, 0x030201], dtype=np.uint32)
    palette = np.full(100, 0x010203, dtype=np.uint32)
    out = np.zeros((64, 64, 3), dtype=">u2")

    def set_dp(r, dd=d, table=lut, n=None):
        return cb.lib.cb_renderer_set_depth_palette(r._h, None if dd is None else C.byref(dd),
                                                    None if table is None else table.ctypes.data,
                                                    (0 if table is None else table.size) if n is None else n)

    def still_usable(r, shape):
        r.render_passes(1)
        hist = r.read_histogram()
        assert hist.shape == shape and int(hist.sum()) == r.read_counters().as_dict()["increments"] > 0
        assert r.depth_palette() is None
        assert cb.lib.cb_renderer_depth_palette_image(r._h, 1.0, 0, out.ctypes.data, None, None) == INVALID

    with cb.Renderer(dims, it, device=0, n_threads=1024) as r:
        assert set_dp(r) == INVALID  # a plain renderer
        still_usable(r, (64, 64))
    with cb.Renderer(dims, [(100, 20), (50, 5)], device=0, n_threads=1024) as r:
        assert set_dp(r) == INVALID  # a channel renderer
        still_usable(r, (2, 64, 64))
    focus_box = cb.FractalDimensions.make(64, 64, -0.2, 0.0, -0.9, -0.7)
    with cb.Renderer(focus_box, cb.IterationControl(300, 20), device=0, n_threads=4096) as r:
        r.set_focus(6, 4, 1)
        assert set_dp(r) == INVALID  # a focused renderer
        still_usable(r, (64, 64))
    with cb.Renderer(dims, it, device=0, n_threads=1024) as r:
        r.set_palette(palette)
        assert set_dp(r) == INVALID  # a palette renderer: colour by escape index and by depth at once is out of scope
        still_usable(r, (3, 64, 64))
        rgb, _, _ = r.palette_image()  # and it is a palette renderer still
        assert rgb.any()
    with cb.Renderer(dims, it, device=0, n_threads=1024) as r:
        r.set_projection(cb.IDENTITY_PROJECTION)
        r.set_depth(d)
        assert set_dp(r) == INVALID  # a renderer that has a depth
        still_usable(r, (5, 64, 64))
        assert r.depth().as_tuple() == d.as_tuple()
    with cb.Renderer(dims, it, device=0, n_threads=1024) as r:
        r.set_projection(cb.IDENTITY_PROJECTION)
        r.render_passes(1)
        assert set_dp(r) == INVALID  # after the first pass
        still_usable(r, (64, 64))
    nan, inf = float("nan"), float("inf")
    with cb.Renderer(dims, it, device=0, n_threads=1024) as r:
        r.set_julia(C_JULIA)
        fresh = r.read_rng_states().copy()
        assert set_dp(r, None) == INVALID and set_dp(r, table=None, n=5) == INVALID
        for n in (0, 4, 6):
            assert set_dp(r, n=n) == INVALID, n  # a table of another length than N
        assert set_dp(r, table=lut | np.uint32(1 << 24)) == INVALID  # as cb_renderer_set_palette: bits 24-31 clear
        for bad in (((nan, 0, 0, 0), 0, 1, 5), ((0, 0, inf, 0), 0, 1, 5), ("cr", nan, 1, 5), ("cr", 0, inf, 5), ("cr", 1, 1, 5),
                    ("cr", 2, 1, 5), ("cr", -1.7e308, 1.7e308, 5)):
            assert set_dp(r, cb.Depth.make(*bad)) == INVALID, bad
        for slices in (0, -4, 257):
            assert set_dp(r, cb.Depth.make("cr", 0, 1, slices), n=max(slices, 0)) == INVALID, slices
        assert r.depth_palette() is None and r.read_histogram().shape == (64, 64)
        r.set_depth_palette(d, lut)
        assert r.depth_palette()[0].as_tuple() == d.as_tuple() and r.julia() == C_JULIA
        assert set_dp(r) == INVALID  # once
        assert cb.lib.cb_renderer_set_depth(r._h, C.byref(d)) == INVALID
        assert cb.lib.cb_renderer_set_palette(r._h, palette.ctypes.data, 100) == INVALID
        assert cb.lib.cb_renderer_set_projection(r._h, good) == INVALID
        assert cb.lib.cb_renderer_set_julia(r._h, good, c_good) == INVALID
        assert cb.lib.cb_renderer_set_focus(r._h, 6, 2, 1, 0) == INVALID
        for variant in (cb.CB_KERNEL_FLAG_ANTI, cb.CB_KERNEL_FULL_ITERATE, cb.CB_KERNEL_TIMED, 9 << 12,
                        cb.CB_KERNEL_POWER(3) | cb.CB_KERNEL_FLAG_BURNING_SHIP):
            assert cb.lib.cb_renderer_render_passes(r._h, 1, variant) == INVALID
        hist = r.read_histogram()
        assert hist.shape == (3, 64, 64) and int(hist.sum()) == 0 and r.read_counters().as_dict()["samples"] == 0
        assert np.array_equal(r.read_rng_states(), fresh)
        # the images of the renders it is not stay refused, and its own refuses what the palette's does
        gray = np.zeros((5, 64, 64), dtype=">u2")
        assert cb.lib.cb_renderer_palette_image(r._h, 1.0, 0, out.ctypes.data, None, None) == INVALID
        assert cb.lib.cb_renderer_depth_image(r._h, 1.0, 0, gray.ctypes.data, None, None) == INVALID
        assert cb.lib.cb_renderer_depth_palette_image(r._h, 1.0, 0, None, None, None) == INVALID
        assert cb.lib.cb_renderer_depth_palette_image(r._h, 1.0, 7, out.ctypes.data, None, None) == INVALID  # no such mode
        r.render_passes(1)  # and it renders
        hist = r.read_histogram()
        assert int(hist.sum()) == r.read_counters().as_dict()["increments"] > 0


def test_depth_palette_launches_refuse_what_they_do_not_define(cb):
    import torch

    dev = torch.device("cuda", 0)
    threads = 256
    dims = cb.FractalDimensions.make(64, 64)
    it = cb.IterationControl(100, 20)
    d_lut = torch.full((256,), 0x010203, dtype=torch.int32, device=dev)
    bufs = plot_harness.Launches(cb, dims, threads, planes=3)
    buf, counters, states = bufs.out, bufs.counters, bufs.states
    torch.cuda.synchronize()
    before = states.cpu().numpy().copy()
    good = (C.c_double * 8)(*cb.IDENTITY_PROJECTION)
    bad_matrix = (C.c_double * 8)(*([float("nan")] + list(cb.IDENTITY_PROJECTION[1:])))
    c_good = (C.c_double * 2)(*C_JULIA)
    d_good = cb.Depth.make("cr", -2.0, 0.5, 5)
    nan, inf = float("nan"), float("inf")

    def draw(variant=0, c=None, p=good, d=d_good, lut=d_lut.data_ptr(), n=None, samples=5, n_threads=threads):
        entries = (d.slices if d is not None else 5) if n is None else n
        return cb.lib.cb_draw_buddhabrot_depth_palette(C.byref(dims), buf.data_ptr(), C.byref(it), p, c,
                                                       None if d is None else C.byref(d), lut, entries & 0xFFFFFFFF,
                                                       states.data_ptr(), n_threads, samples, counters.data_ptr(), variant,
                                                       None)

    for c in (None, c_good):
        for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
            assert draw(base, c=c, d=None) == INVALID and draw(base, c=c, lut=None) == INVALID
            for n in (0, 4, 6, 256):
                assert draw(base, c=c, n=n) == INVALID, n
            for bad in (((0, nan, 0, 0), 0, 1, 1), ((0, 0, 0, -inf), 0, 1, 1), ("cr", nan, 1, 1), ("cr", 0, nan, 1),
                        ("cr", -inf, 1, 1), ("cr", 1, 1, 1), ("cr", 2, 1, 1), ("cr", 0, 1, 0), ("cr", 0, 1, 257),
                        ("cr", -1.7e308, 1.7e308, 1)):
                assert draw(base, c=c, d=cb.Depth.make(*bad)) == INVALID, bad
            assert draw(base, c=c, p=None) == INVALID and draw(base, c=c, p=bad_matrix) == INVALID
        power3 = cb.CB_KERNEL_POWER(3)
        for variant in (cb.CB_KERNEL_FLAG_ANTI, cb.CB_KERNEL_SIMPLE | cb.CB_KERNEL_FLAG_ANTI, cb.CB_KERNEL_TIMED,
                        cb.CB_KERNEL_FULL_ITERATE, cb.CB_KERNEL_FLAG_DRAIN, power3 | cb.CB_KERNEL_FLAG_BURNING_SHIP,
                        power3 | cb.CB_KERNEL_FORMULA(2), cb.CB_KERNEL_FORMULA(2) | cb.CB_KERNEL_FLAG_BURNING_SHIP,
                        2 << 12, 9 << 12, 6 << 16):
            assert draw(variant, c=c) == INVALID, variant
    for c in ((2.5, 0.0), (0.0, -2.0000001), (nan, 0.0), (0.0, inf)):
        for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
            assert draw(base, c=(C.c_double * 2)(*c)) == INVALID, c
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0 and int(counters.sum()) == 0
    assert np.array_equal(states.cpu().numpy(), before)
    for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):  # no threads or no samples: nothing launched, success
        for c in (None, c_good):
            assert draw(base, c=c, samples=0) == 0 and draw(base, c=c, n_threads=0) == 0
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0 and int(counters.sum()) == 0 and np.array_equal(states.cpu().numpy(), before)
    assert draw(cb.CB_KERNEL_DEFAULT) == 0  # and what is defined renders
    assert int(buf.sum()) == bufs.read_counters()["increments"] > 0


def host_image(cb, hist, gamma):
    """"Palette render", Image, on the host: the three planes as one w x 3h image, then interleaved -> ([h, w, 3]
    big-endian u16, max, scale)."""
    planes, h, w = hist.shape
    gray, mx, scale = cb.set_grayscale_pixels(hist.reshape(3 * h, w), gamma)
    return np.ascontiguousarray(gray.reshape(3, h, w).transpose(1, 2, 0)).astype(">u2"), mx, scale


@pytest.fixture(scope="module")
def rendered(cb):
    """One renderer with a depth palette and a few passes in it, and its histogram."""
    dims = cb.FractalDimensions.make(W, H)
    with cb.Renderer(dims, cb.IterationControl(MAX, MIN), device=0, n_threads=THREADS) as r:
        r.set_projection(cb.IDENTITY_PROJECTION)
        r.set_depth_palette(("cr", -2.0, 0.5, 5), [0x0000FF, 0x003F7F, 0x1F7F00, 0x7F0000, 0xFF0000])
        r.render_passes(3)
        yield r, r.read_histogram()


@pytest.mark.parametrize("mode", ["CB_TONE_LUT", "CB_TONE_THRESHOLDS", "CB_TONE_AUTO"])
@pytest.mark.parametrize("gamma", [1.0, 2.2, -1.0])
def test_image_is_the_tone_map_against_the_common_maximum(cb, rendered, mode, gamma):
    r, hist = rendered
    assert len({int(hist[j].max()) for j in range(3)}) == 3  # three different maxima: a common one shows
    rgb, mx, scale = r.depth_palette_image(gamma, getattr(cb, mode))
    assert rgb.shape == (H, W, 3) and mx == int(hist.max())
    want = np.array([cb.tone_value(int(v), mx, gamma) for v in hist.reshape(-1)], dtype=np.uint16).reshape(hist.shape)
    assert np.array_equal(rgb.astype(np.uint16), want.transpose(1, 2, 0))
    body, want_max, want_scale = host_image(cb, hist, gamma)
    assert (mx, scale) == (want_max, want_scale) and rgb.tobytes() == body.tobytes()
    # (the brightest value is cb_tone_value(max, max, gamma): the reference's scale-then-multiply may land one below 65535)
    assert int(rgb.max()) == cb.tone_value(mx, mx, gamma) >= 65534 or gamma <= 0


def test_planes_tone_map_with_their_own_maximum(cb, rendered):
    r, hist = rendered
    for j in range(3):
        gray, mx, _ = r.grayscale_image(1.0, plane=j)
        want, want_max, _ = cb.set_grayscale_pixels(hist[j], 1.0)
        assert mx == want_max == int(hist[j].max()) and np.array_equal(gray.astype(np.uint16), want)
    out = np.zeros((H, W), dtype=">u2")
    assert cb.lib.cb_renderer_grayscale_plane(r._h, 3, 1.0, 0, out.ctypes.data, None, None) == INVALID


# ---- 4. the binary --------------------------------------------------------------------------------------------------------

STOPS_TEXT = "0:000030,2:ff8000,4:ffffff"
STOPS = [(0, 0x00, 0x00, 0x30), (2, 0xFF, 0x80, 0x00), (4, 0xFF, 0xFF, 0xFF)]


def read_ppm(path, w, h):
    with open(path, "rb") as f:
        data = f.read()
    header = b"P6\n%d %d\n65535\n" % (w, h)
    assert data[:len(header)] == header and len(data) == len(header) + 6 * w * h  # one P6 of w x h, 16 bits
    return data, np.frombuffer(data, dtype=">u2", offset=len(header)).reshape(h, w, 3)


def test_cli_image_buffer_stats_and_kernels(cb, exe, ref, tmp_path):
    common = ["--depth", "cr:-2:0.5:5", "--depth-palette", STOPS_TEXT, "-g", "2.2", "-w", "64", "-h", "48", "-m", "300",
              "-c", "20", "--passes", "2"]
    lut = cb.palette_from_stops(STOPS, 5)
    buf, ppm, host_ppm = str(tmp_path / "d.bin"), str(tmp_path / "d.ppm"), str(tmp_path / "host.ppm")
    r = run(exe, *common, "-s", buf, "--stats", "-o", ppm)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Saving image." in r.stdout and "Done! Output image saved: %s" % ppm in r.stdout
    lines = r.stderr.strip().split("\n")
    assert [float.fromhex(v) for v in json.loads(lines[0])["projection"]] == [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]
    assert json.loads(lines[1]) == {"depth": {"row": ["0x0p+0", "0x0p+0", "0x1p+0", "0x0p+0"], "min": "-0x1p+1",
                                              "max": "0x1p-1", "slices": 5}}
    assert json.loads(lines[2]) == {"depth_palette": [[0, "000030"], [2, "ff8000"], [4, "ffffff"]]}
    hist = read_state_file(buf, 48, 64, planes=3)  # the header says 3 planes, whatever N is
    data, pixels = read_ppm(ppm, 64, 48)
    body, mx, scale = host_image(cb, hist, 2.2)
    assert "Max value: %d, scale: %f" % (mx, scale) in r.stdout and mx == int(hist.max()) > 0
    assert np.array_equal(pixels, body) and all(p.any() for p in hist)
    assert run(exe, *common, "--tonemap", "host", "-o", host_ppm).returncode == 0
    with open(host_ppm, "rb") as f:
        assert f.read() == data  # the reference's host loop gives the same file
    # and the buffer is the restatement's
    ref_hist, rc = plot.draw(ref, 64, 48, 300, 20, 512 * 512, [100], depth=("cr", -2.0, 0.5, 5), lut=lut,
                             omp_threads=omp_threads())
    stats = json.loads(lines[-1])
    assert stats["status"] == 0 and {k: stats[k] for k in SAME} == rc and np.array_equal(hist, ref_hist)
    # --kernel picks the kernel: the product kernel (20) consults the interior map and skips steps, the lock-step kernel
    # (21) does neither; both write the same buffer
    assert stats["skipped_steps"] > 0 and min(stats["interior_map_levels"]) >= 1
    simple_buf = str(tmp_path / "simple.bin")
    r2 = run(exe, *common, "--kernel", "simple", "-s", simple_buf, "--stats", "-o", os.devnull)
    assert r2.returncode == 0, r2.stdout + r2.stderr
    simple = json.loads(r2.stderr.strip().split("\n")[-1])
    assert simple["skipped_steps"] == 0 and simple["interior_map_levels"] == [0]
    assert {k: simple[k] for k in SAME} == rc and np.array_equal(read_state_file(simple_buf, 48, 64, planes=3), hist)


def test_cli_resumes_with_julia_power_and_seed(cb, exe, tmp_path):
    common = ["--depth", "zi:-1:1:256", "--depth-palette", "0:000030,128:ff8000,255:ffffff", "--julia", "0.3,0.5",
              "--power", "3", "--seed", "99", "-w", "64", "-h", "48", "-m", "100", "-c", "5"]
    one_buf, one_side, one_ppm = str(tmp_path / "one.bin"), str(tmp_path / "one.rng"), str(tmp_path / "one.ppm")
    assert run(exe, *common, "--passes", "2", "-s", one_buf, "--rng-state", one_side, "-o", one_ppm).returncode == 0
    read_ppm(one_ppm, 64, 48)
    assert read_state_file(one_buf, 48, 64, planes=3).any()
    buf, side, ppm = str(tmp_path / "two.bin"), str(tmp_path / "two.rng"), str(tmp_path / "two.ppm")
    assert run(exe, *common, "--passes", "1", "-s", buf, "--rng-state", side, "-o", os.devnull).returncode == 0
    r2 = run(exe, *common, "--passes", "1", "-s", buf, "--rng-state", side, "-o", ppm)
    assert r2.returncode == 0 and "Continuing the sample stream after 1 passes." in r2.stdout, r2.stdout
    for a, b in ((buf, one_buf), (side, one_side), (ppm, one_ppm)):
        with open(a, "rb") as fa, open(b, "rb") as fb:
            assert fa.read() == fb.read(), a
